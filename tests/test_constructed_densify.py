"""(CPU) tests/constructed_densify.py keeps its promises.

Every scene is run through oracle.densify_oracle.densify_and_prune (pinned to the reference by the
golden files): the row count is the builder's P', every copied tensor is the builder's gather of
its source rows bit for bit, moments are zero on clone and child rows, the step is kept.  That is
what makes the counts "exact by construction" and not whatever the oracle says.  Each scene's purpose
is asserted too, so that a later edit cannot hollow a case out.
"""
import numpy as np
import pytest
import torch

import constructed_densify as CD
from constructed_densify import K
from oracle import densify_oracle as DO
from test_densify import _check_model_structure, _model_from


def _run_oracle(case, f_rest_k=15, with_state=True):
    arrays = case.arrays(f_rest_k)
    m = _model_from(arrays, "cpu", with_state)
    torch.manual_seed(3)
    DO.densify_and_prune(m, *case.args(), case.N)
    _check_model_structure(m)
    assert m._xyz.shape[0] == case.P_out
    CD.assert_outputs_from_builder(case, arrays, m, CD.NAMES if with_state else ())
    return arrays, m


def _children_follow_their_parents(case, arrays, m):
    """child scaling = log(exp(s) / (0.8 N)) of its source row, within the golden bound"""
    n_copy = int(case.totals[0] + case.totals[1])
    src = case.src_rows[n_copy:]
    want = np.log(np.exp(arrays["scaling"][src].astype(np.float64)) / (0.8 * case.N))
    np.testing.assert_allclose(m._scaling.detach().numpy()[n_copy:], want, rtol=1e-6, atol=1e-6)


def test_kind_table_decisions():
    """The verdict on every kind, written out by hand for N = 2 with a screen size."""
    clone, split, ka, kb, kc = CD.classify_kinds(2, 20.0)
    want = {  # kind: (clone, split, kept original, kept clone, kept children)
        "keep": (0, 0, 1, 0, 0), "clone": (1, 0, 1, 1, 0), "clone_transp": (1, 0, 0, 0, 0),
        "split": (0, 1, 0, 0, 1), "split_transp": (0, 1, 0, 0, 0), "split_child_big": (0, 1, 0, 0, 0),
        "split_parent_big": (0, 1, 0, 0, 1), "big_nograd": (0, 0, 0, 0, 0), "transp": (0, 0, 0, 0, 0),
        "nan_grad": (0, 0, 1, 0, 0), "nan_grad_large": (0, 0, 1, 0, 0), "inf_small": (1, 0, 1, 1, 0),
        "inf_large": (0, 1, 0, 0, 1), "neg_small": (1, 0, 1, 1, 0), "neg_large": (0, 0, 1, 0, 0),
        "tie_g_in_small": (1, 0, 1, 1, 0), "tie_g_in_large": (0, 1, 0, 0, 1), "tie_g_out_small": (0, 0, 1, 0, 0),
        "tie_g_out_large": (0, 0, 1, 0, 0), "tie_s_zero": (1, 0, 1, 1, 0), "tie_s_eps": (0, 1, 0, 0, 1),
        "tie_op_zero": (0, 0, 1, 0, 0), "tie_op_subnormal": (0, 0, 1, 0, 0), "tie_op_below": (0, 0, 0, 0, 0),
        "tie_op_zero_clone": (1, 0, 1, 1, 0), "tie_op_below_split": (0, 1, 0, 0, 0),
    }
    assert set(want) == set(CD.KIND_NAMES)
    for n, w in want.items():
        i = K[n]
        assert (clone[i], split[i], ka[i], kb[i], kc[i]) == tuple(bool(x) for x in w), n
    # without a screen size nothing is pruned by size; with a negative one everything is
    _, _, ka, _, kc = CD.classify_kinds(2, None)
    assert ka[K["big_nograd"]] and kc[K["split_child_big"]]
    _, split, ka, kb, kc = CD.classify_kinds(2, -1.0)
    assert split.any() and not (ka.any() or kb.any() or kc.any())
    # N = 1: the children (s / 0.8) are larger than the parent, so an oversize parent has oversize children
    assert not CD.classify_kinds(1, 20.0)[4][K["split_parent_big"]]
    assert CD.classify_kinds(3, 20.0)[4][K["split_parent_big"]]


def test_tie_inputs_are_the_ties():
    c = CD.edges_scene()
    accum, denom, opacity, scaling = c.decision_inputs()
    g = (accum / np.where(denom == 0, 1, denom))[:, 0]
    m = c.kind_mask("tie_g_in_small", "tie_g_in_large")
    assert m.any() and np.all(g[m] == np.float32(2e-4)) and np.all(g[m].astype(np.float64) < 2e-4)
    m = c.kind_mask("tie_g_out_small", "tie_g_out_large")
    assert m.any() and np.all(np.nextafter(g[m], np.float32(1)) == np.float32(2e-4))
    assert np.all(scaling[c.kind_mask("tie_s_zero")].max(1) == 0.0)
    assert np.all(scaling[c.kind_mask("tie_s_eps")].max(1) == np.float32(1e-6))
    assert np.all(opacity[c.kind_mask("tie_op_zero", "tie_op_zero_clone")] == 0.0)
    sub = opacity[c.kind_mask("tie_op_subnormal")]
    assert sub.size and np.all(sub < 0) and np.all(np.nextafter(sub, np.float32(1)) == 0.0)
    t = torch.tensor(opacity)
    kept = torch.sigmoid(t) >= 0.5  # torch's own float32 sigmoid on these rows
    assert kept[torch.tensor(c.kind_mask("tie_op_zero", "tie_op_subnormal"))].all()
    assert not kept[torch.tensor(c.kind_mask("tie_op_below", "tie_op_below_split"))].any()
    assert np.all(scaling.max(1) == scaling[np.arange(c.P), np.arange(c.P) % 3])  # the max moves over the axes


@pytest.mark.parametrize("kind", ["keep", "clone", "split", "split_child_big"])
def test_lanes_scene(kind):
    c = CD.lanes_scene(kind)
    at = np.array(c.props["at"])
    assert list(at[:5]) == [0, 63, 64, 255, 256] and at[5] == c.P - 1 and c.blocks == 2
    other = np.ones(c.P, bool)
    other[at] = False
    assert not (c.keep_a | c.keep_b | c.split | c.keep_c)[other].any()
    want = {"keep": (6, 0, 0, 0), "clone": (6, 6, 0, 0), "split": (0, 0, 6, 6), "split_child_big": (0, 0, 6, 0)}[kind]
    assert tuple(c.totals) == want
    assert tuple(c.block_counts[0]) == tuple(4 * (w > 0) for w in want)
    _run_oracle(c)


def test_dead_wave_scene():
    c = CD.dead_wave_scene()
    lo, hi = c.props["wave"]
    assert lo % 64 == 0 and hi - lo == 64 and lo % 256 != 0
    assert not (c.keep_a | c.keep_b | c.keep_c)[lo:hi].any() and c.split[lo:hi].any()
    for w0 in (lo - 64, hi):
        assert c.keep_a[w0:w0 + 64].any() and c.keep_b[w0:w0 + 64].any() and c.keep_c[w0:w0 + 64].any()
    _run_oracle(c)


def test_split_wave_scene():
    c = CD.split_wave_scene()
    lo, hi = c.props["wave"]
    assert lo % 64 == 0 and hi - lo == 64 and c.keep_c[lo:hi].all() and c.split[lo:hi].all()
    arrays, m = _run_oracle(c, f_rest_k=15)
    assert arrays["f_rest"][0].size == 45
    _children_follow_their_parents(c, arrays, m)


def test_clone_block_split_block_scene():
    c = CD.clone_block_split_block_scene()
    assert c.P % 64 != 0 and c.blocks == 4
    assert tuple(c.block_counts[1]) == (256, 256, 0, 0) and tuple(c.block_counts[2]) == (0, 0, 256, 256)
    assert np.array_equal(c.block_bases[2] - c.block_bases[1], [256, 256, 0, 0])
    assert np.array_equal(c.block_bases[3] - c.block_bases[2], [0, 0, 256, 256])
    assert c.block_counts[0].all() and c.block_counts[3].all()
    _run_oracle(c)


@pytest.mark.parametrize("which", ["first", "last"])
def test_one_block_only_scene(which):
    c = CD.one_block_only_scene(which)
    b = 0 if which == "first" else c.blocks - 1
    others = np.arange(c.blocks) != b
    assert c.blocks == 6 and c.block_counts[b, 1:].all()
    assert not c.block_counts[others, 1:].any() and c.block_counts[others, 0].all()
    _run_oracle(c)


@pytest.mark.parametrize("which", CD.EMPTY_CLASS)
def test_empty_class_scene(which):
    c = CD.empty_class_scene(which)
    t = c.totals
    if which == "no_split":
        assert t[2] == 0 and t[3] == 0 and t[0] > 0 and t[1] > 0
    elif which == "no_clone":
        assert not c.clone.any() and t[1] == 0 and t[3] > 0 and t[0] > 0
    elif which == "no_kept_child":
        assert t[3] == 0 < t[2] and t[0] > 0 and t[1] > 0
    else:
        assert c.P_out == 0 and not t[[0, 1, 3]].any() and t[2] > 0
        assert (which == "nothing_by_screen") == (c.screen == -1.0)
    arrays, m = _run_oracle(c)
    if c.P_out == 0:
        for name, attr in zip(DO.NAMES, DO.ATTRS):
            p = getattr(m, attr)
            assert tuple(p.shape) == (0,) + arrays[name].shape[1:]
            assert m.optimizer.state[p]["exp_avg"].shape == p.shape


def test_no_split_draws_nothing():
    """The oracle (as the reference) draws normal() of zero rows: the generator does not move."""
    c = CD.empty_class_scene("no_split")
    m = _model_from(c.arrays(), "cpu")
    torch.manual_seed(5)
    before = torch.get_rng_state()
    DO.densify_and_prune(m, *c.args(), c.N)
    assert torch.equal(before, torch.get_rng_state())


@pytest.mark.parametrize("N,screen", [(2, 20.0), (1, 20.0), (3, 20.0), (2, None), (3, -1.0)])
def test_edges_scene(N, screen):
    c = CD.edges_scene(N, screen)
    assert c.P <= 330 and set(c.kinds) == set(range(len(CD.KIND_NAMES)))
    arrays, m = _run_oracle(c)
    _children_follow_their_parents(c, arrays, m)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_sized_scene(P, N):
    c = CD.sized_scene(P, N, (20.0, None, -1.0)[(P + N) % 3])
    assert c.P == P
    _run_oracle(c, f_rest_k=(0, 3, 15)[P % 3], with_state=P % 2 == 1)


def test_scan_pattern_is_not_uniform_over_a_thread_range():
    """At 1025 blocks (per 2) thread t owns blocks 2t, 2t + 1, thread 512 owns block 1024 alone and
    threads 513.. are idle.  The pattern makes a block's base depend on its range's earlier blocks:
    dropping the carry inside a range changes bases that rows use."""
    P = 262_145
    c = CD.scan_scene(P, "blocks")
    assert c.blocks == 1025 and c.per == 2
    assert CD.scan_scene(262_144, "blocks").per == 1
    bc = c.block_counts
    # odd threads: first block all clones or all splits, a mix behind it that uses every base
    first, second = bc[2:1024:4], bc[3:1024:4]
    assert np.all((first[:, 1] == 256) | (first[:, 2] == 256)) and second.all()
    # even threads: nothing, then a dense block
    assert not bc[0:1024:4].any() and bc[1:1024:4].any(1).all()
    # the block thread 512 owns alone: the model's last row, a split
    assert tuple(bc[1024]) == (0, 0, 1, 1) and c.split[P - 1]
    no_carry = c.block_bases.copy()
    no_carry[1::2] = no_carry[0:-1:2]  # what the scan gives without `run += c`
    used = bc > 0
    assert (no_carry != c.block_bases)[used].sum() > 500
    # 2049 blocks: per 3, thread 682 owns the last three blocks, the first of them whole
    c3 = CD.scan_scene(524_289, "blocks")
    assert c3.per == 3 and c3.blocks == 2049 and c3.blocks - 682 * 3 == 3
    assert CD.scan_scene(524_288, "blocks").per == 2
