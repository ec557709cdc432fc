"""densify_and_prune inputs whose outcome is exact by construction (CPU only, seeded).

Every other densify case is a random draw, so no comparison ever sits on its bound, no class is
ever empty and no class ever fills a wave or a 256-block.  Here a model is assembled from ROW
KINDS (the KINDS table below): a kind fixes the four numbers the decision reads (accum, denom,
the largest scaling, the raw opacity); everything else in the row is random and unique, so an
output row identifies its source row.

The call's scalars make the ties exact on any math library:
    percent_dense 0.01 * extent 100.0 == 1.0 (pd_ext),  0.1 * extent == 10.0 (big_ext),
    grad threshold 2e-4 (float32(2e-4) < 2e-4: torch compares in float32),  min_opacity 0.5,
    exp(0.0) == 1.0,  sigmoid(0.0) == 0.5,  g = accum / 1 = accum.
Every kind either sits exactly on a bound (the "tie_*" kinds) or keeps a margin that no float32
math library can cross; classify_kinds() asserts the margins:
    max scale vs pd_ext 1.0   : tie at scaling 0.0, else |exp(s) - 1| >= 5e-7 (4 float32 steps)
    sigmoid vs 0.5            : tie at opacity 0.0 (and -1.4e-45, see below), else >= 2e-7
    max scale vs big_ext 10.0 : >= 1 % (parents and children: exp(log(s * inv)) is no round trip, so
                                the child bound has no exact tie; "split_child_big" / "split_parent_big"
                                keep their margin on either side of it)
"One float32 step below opacity 0.0" is the subnormal -1.4e-45, whose sigmoid is 0.5 in float32
(1 + exp(1.4e-45) == 2): it is KEPT, and is in the table as tie_op_subnormal.  The first raw
opacity that is pruned on every library is a few float32 steps of the sigmoid further, -1e-6
(sigmoid 0.5 - 2.5e-7, 8 steps below 0.5): tie_op_below.

From the kinds alone (numpy, never the oracle or the HIP library) a Case carries: the per-row
classes, the four totals {kept originals, kept clones, split parents, kept split parents}, their
per-256-block counts and exclusive block bases, P' = t0 + t1 + N * t3, and the source row of every
output row in the layout [kept originals | kept clones | children, k-major].
tests/test_constructed_densify.py checks these promises against the oracle on the CPU;
tests/test_gpu_constructed_densify.py runs the HIP path on the same cases.

Reference quirk kept out of the scenes: with exactly ONE row left before the final prune, the
reference's prune_mask.squeeze() is 0-d and indexing with it adds a dimension.  No scene here leaves
exactly one row at that point (Case.rows_before_prune != 1 is asserted).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

BLOCK = 256          # Gaussians per classify / emit block (gs_densify.hip DENS_T)
WAVE = 64
SCAN_THREADS = 1024  # k_dens_scan: one block; thread t owns ceil(blocks / 1024) classify blocks
PERCENT_DENSE = 0.01  # tests/test_densify.py _model_from
EXTENT = 100.0
THR = 2e-4
MIN_OPACITY = 0.5
PD_EXT = PERCENT_DENSE * EXTENT
BIG_EXT = 0.1 * EXTENT
assert PD_EXT == 1.0 and BIG_EXT == 10.0
THR32 = np.float32(THR)
assert float(THR32) < THR
THR32_BELOW = np.nextafter(THR32, np.float32(0.0))
SUBNORMAL = float(np.nextafter(np.float32(0.0), np.float32(-1.0)))  # -1.4e-45

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")

# kind: (accum, denom, largest scaling (raw, i.e. log), raw opacity)
_L = lambda s: float(np.float32(np.log(s)))  # noqa: E731
KINDS = {
    "keep":              (0.0, 1.0, _L(0.1), 2.0),
    "clone":             (4e-4, 1.0, _L(0.1), 2.0),
    "clone_transp":      (4e-4, 1.0, _L(0.1), -2.0),   # neither the original nor the clone survives
    "split":             (4e-4, 1.0, _L(2.0), 2.0),
    "split_transp":      (4e-4, 1.0, _L(2.0), -2.0),   # in totals[2]: its stds rows are drawn; no children
    "split_child_big":   (4e-4, 1.0, _L(100.0), 2.0),  # children 100 / (0.8 N) > 10 for N <= 3
    "split_parent_big":  (4e-4, 1.0, _L(12.0), 2.0),   # 12 > 10; children 7.5 (N 2), 5 (N 3); 15 for N 1
    "big_nograd":        (0.0, 1.0, _L(12.0), 2.0),    # pruned with a screen size, kept with None
    "transp":            (0.0, 1.0, _L(0.1), -2.0),
    "nan_grad":          (0.0, 0.0, _L(0.1), 2.0),     # 0 / 0 -> NaN -> 0
    "nan_grad_large":    (0.0, 0.0, _L(2.0), 2.0),
    "inf_small":         (1.0, 0.0, _L(0.1), 2.0),     # +inf: clone
    "inf_large":         (1.0, 0.0, _L(2.0), 2.0),     # +inf: split
    "neg_small":         (-4e-4, 1.0, _L(0.1), 2.0),   # clone by |g|
    "neg_large":         (-4e-4, 1.0, _L(2.0), 2.0),   # never split: kept
    "tie_g_in_small":    (float(THR32), 1.0, _L(0.1), 2.0),        # g == float32(thr): clone
    "tie_g_in_large":    (float(THR32), 1.0, _L(2.0), 2.0),        # split
    "tie_g_out_small":   (float(THR32_BELOW), 1.0, _L(0.1), 2.0),  # one float32 step below: kept
    "tie_g_out_large":   (float(THR32_BELOW), 1.0, _L(2.0), 2.0),
    "tie_s_zero":        (4e-4, 1.0, 0.0, 2.0),        # exp(0) == 1 <= pd_ext: clone, not split
    "tie_s_eps":         (4e-4, 1.0, 1e-6, 2.0),       # exp(1e-6) > 1: split
    "tie_op_zero":       (0.0, 1.0, _L(0.1), 0.0),     # sigmoid(0) == 0.5, not < 0.5: kept
    "tie_op_subnormal":  (0.0, 1.0, _L(0.1), SUBNORMAL),  # sigmoid == 0.5 in float32: kept
    "tie_op_below":      (0.0, 1.0, _L(0.1), -1e-6),   # pruned
    "tie_op_zero_clone": (4e-4, 1.0, _L(0.1), 0.0),    # original and clone kept
    "tie_op_below_split": (4e-4, 1.0, _L(2.0), -1e-6),  # split parent without children
}
KIND_NAMES = tuple(KINDS)
K = {n: i for i, n in enumerate(KIND_NAMES)}
_TABLE = np.array([KINDS[n] for n in KIND_NAMES], np.float64)


def classify_kinds(N: int, screen):
    """Per kind: (clone, split, keep_a, keep_b, keep_c) for a call with N children and
    max_screen_size `screen`, with the margins of the module docstring asserted."""
    accum, denom = _TABLE[:, 0].astype(np.float32), _TABLE[:, 1].astype(np.float32)
    logs, op = _TABLE[:, 2].astype(np.float32).astype(np.float64), _TABLE[:, 3].astype(np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = accum / denom                                   # float32, exact for denom 1
    g = np.where(np.isnan(g), np.float32(0.0), g)
    over_abs, over = np.abs(g) >= THR32, g >= THR32          # float32 compares: no library involved
    ms = np.exp(logs)
    assert np.all((logs == 0.0) | (np.abs(ms - 1.0) >= 5e-7))
    small = ms <= PD_EXT
    clone, split = over_abs & small, over & ~small
    o = 1.0 / (1.0 + np.exp(-op))
    tie_o = np.abs(op) < 1e-30
    assert np.all(o[tie_o] == 0.5) and np.all(np.abs(o[~tie_o] - 0.5) >= 2e-7)
    transp = o < MIN_OPACITY
    has_screen = bool(screen)                               # the reference's `if max_screen_size:`
    everything = has_screen and screen < 0                  # max_radii2D (all 0 by then) > negative
    inv = float(np.float32(1.0) / np.float32(0.8 * N))
    cms = ms * inv
    assert np.all(np.abs(ms / BIG_EXT - 1.0) > 1e-2) and np.all(np.abs(cms[split] / BIG_EXT - 1.0) > 1e-2)
    prune = transp | (has_screen & (everything | (ms > BIG_EXT)))
    cprune = transp | (has_screen & (everything | (cms > BIG_EXT)))
    return clone, split, ~split & ~prune, clone & ~prune, split & ~cprune


@dataclass
class Case:
    name: str
    kinds: np.ndarray            # [P] index into KIND_NAMES
    N: int
    screen: object               # max_screen_size: float or None
    clone: np.ndarray            # [P] bool, the classes of every row
    split: np.ndarray
    keep_a: np.ndarray
    keep_b: np.ndarray
    keep_c: np.ndarray
    totals: np.ndarray           # [4] {kept originals, kept clones, split parents, kept split parents}
    block_counts: np.ndarray     # [blocks, 4]
    block_bases: np.ndarray      # [blocks, 4] exclusive
    P_out: int
    src_rows: np.ndarray         # [P_out] source row of every output row
    props: dict = field(default_factory=dict)

    @property
    def P(self):
        return len(self.kinds)

    @property
    def blocks(self):
        return (self.P + BLOCK - 1) // BLOCK

    @property
    def per(self):
        """classify blocks per k_dens_scan thread"""
        return (self.blocks + SCAN_THREADS - 1) // SCAN_THREADS

    @property
    def rows_before_prune(self):
        return self.P + int(self.clone.sum()) + (self.N - 1) * int(self.split.sum())

    @property
    def n_orig(self):
        return int(self.totals[0])

    @property
    def n_new(self):
        """clone and child rows: zero moments"""
        return self.P_out - int(self.totals[0])

    def args(self):
        """(max_grad, min_opacity, extent, max_screen_size) of the call"""
        return THR, MIN_OPACITY, EXTENT, self.screen

    def kind_mask(self, *names):
        return np.isin(self.kinds, [K[n] for n in names])

    def decision_inputs(self):
        """The four arrays the decision reads: accum [P,1], denom [P,1], opacity [P,1], scaling
        [P,3] (float32).  The largest scaling sits on axis row % 3, the others at 1/2 and 1/4."""
        P = self.P
        t = _TABLE[self.kinds]
        accum = t[:, 0].astype(np.float32).reshape(P, 1)
        denom = t[:, 1].astype(np.float32).reshape(P, 1)
        opacity = t[:, 3].astype(np.float32).reshape(P, 1)
        logs = t[:, 2].astype(np.float32)
        off = np.array([0.0, np.log(0.5), np.log(0.25)], np.float32)
        scaling = logs[:, None] + off[(np.arange(3)[None, :] - (np.arange(P) % 3)[:, None]) % 3]
        assert scaling.dtype == np.float32 and np.array_equal(scaling.max(1), logs)
        return accum, denom, opacity, scaling

    def arrays(self, f_rest_k: int = 15, seed: int = 0):
        """The dict tests/test_densify.py _model_from takes (parameters, Adam moments, statistics)."""
        P = self.P
        rng = np.random.default_rng(seed + 7919 * P)
        accum, denom, opacity, scaling = self.decision_inputs()
        d = {
            "xyz": rng.standard_normal((P, 3), np.float32),
            "f_dc": rng.standard_normal((P, 1, 3), np.float32),
            "f_rest": rng.standard_normal((P, f_rest_k, 3), np.float32),
            "opacity": opacity,
            "scaling": scaling,
            "rotation": rng.standard_normal((P, 4), np.float32),
        }
        for n in NAMES:
            d[f"{n}_exp_avg"] = rng.standard_normal(d[n].shape, np.float32) * np.float32(1e-3)
            d[f"{n}_exp_avg_sq"] = rng.random(d[n].shape, np.float32) * np.float32(1e-6)
        d["accum"], d["denom"] = accum, denom
        d["max_radii2D"] = rng.integers(0, 40, (P,)).astype(np.float32)  # re-zeroed before it is read
        return d


def make_case(name: str, kinds, N: int = 2, screen=20.0, **props) -> Case:
    kinds = np.asarray(kinds, np.int64)
    P = len(kinds)
    assert P > 0
    cls = [c[kinds] for c in classify_kinds(N, screen)]
    clone, split, keep_a, keep_b, keep_c = cls
    blocks = (P + BLOCK - 1) // BLOCK
    counted = np.zeros((blocks * BLOCK, 4), np.int64)
    counted[:P] = np.stack([keep_a, keep_b, split, keep_c], 1)
    block_counts = counted.reshape(blocks, BLOCK, 4).sum(1)
    block_bases = np.cumsum(block_counts, 0) - block_counts
    totals = block_counts.sum(0)
    rows = np.arange(P)
    src_rows = np.concatenate([rows[keep_a], rows[keep_b], np.tile(rows[keep_c], N)])
    P_out = int(totals[0] + totals[1] + N * totals[3])
    assert len(src_rows) == P_out
    c = Case(name, kinds, N, screen, clone, split, keep_a, keep_b, keep_c, totals, block_counts, block_bases,
             P_out, src_rows, dict(props))
    assert c.rows_before_prune != 1, "the reference's 0-d prune mask (module docstring)"
    return c


# ---------------------------------------------------------------- kind patterns

EVERY_KIND = np.arange(len(KIND_NAMES))
# no class at all with a screen size set: nothing is written for such a row
DEAD = np.array([K[n] for n in ("transp", "clone_transp", "split_transp", "split_child_big", "tie_op_below",
                                "tie_op_below_split", "big_nograd")])
MIXED = np.array([K[n] for n in ("keep", "clone", "split", "transp", "clone_transp", "split_transp",
                                 "split_child_big", "split_parent_big", "big_nograd", "nan_grad", "neg_small",
                                 "neg_large", "inf_small", "inf_large")])


def mix(P, seed, pool=MIXED):
    return pool[np.random.default_rng(seed).integers(0, len(pool), P)]


def _filled(P, kind):
    return np.full(P, K[kind] if isinstance(kind, str) else kind, np.int64)


LANES = (0, 63, 64, 255, 256)


def lanes_scene(kind, N=2, screen=20.0):
    """One row of `kind` on lanes 0, 63, 64, 255, 256 and on the last row; nothing else has a class."""
    P = 300
    k = _filled(P, "transp")
    at = list(LANES) + [P - 1]
    k[at] = K[kind]
    return make_case(f"lanes_{kind}", k, N, screen, at=at, kind=kind)


def dead_wave_scene(N=2, screen=20.0):
    """Wave 1 of block 1 (rows 320..383) keeps no row of any class; waves around it do."""
    k = mix(700, 1)
    k[320:384] = mix(64, 2, DEAD)
    return make_case("dead_wave", k, N, screen, wave=(320, 384))


def split_wave_scene(N=2, screen=20.0):
    """Rows 128..191 (one wave) all split with kept children."""
    k = mix(450, 3)
    k[128:192] = K["split"]
    return make_case("split_wave", k, N, screen, wave=(128, 192))


def clone_block_split_block_scene(N=2, screen=20.0):
    """Block 1 all clones, block 2 all splits, mixed blocks around them; P no multiple of 64."""
    k = mix(4 * BLOCK - 17, 4)
    k[BLOCK:2 * BLOCK] = K["clone"]
    k[2 * BLOCK:3 * BLOCK] = K["split"]
    return make_case("clone_block_split_block", k, N, screen)


def one_block_only_scene(which, N=2, screen=20.0):
    """Clones and splits in the first (last) block only; the other blocks hold keep / transp rows."""
    P = 5 * BLOCK + 100
    k = mix(P, 5, np.array([K["keep"], K["transp"], K["nan_grad"]]))
    lo, hi = (0, BLOCK) if which == "first" else (5 * BLOCK, P)
    k[lo:hi] = mix(hi - lo, 6, np.array([K["clone"], K["split"], K["split_parent_big"], K["inf_small"]]))
    return make_case(f"{which}_block_only", k, N, screen, rows=(lo, hi))


NO_SPLIT = np.array([K[n] for n in ("keep", "clone", "clone_transp", "transp", "big_nograd", "nan_grad",
                                    "nan_grad_large", "neg_small", "neg_large", "inf_small", "tie_g_in_small",
                                    "tie_g_out_large", "tie_s_zero", "tie_op_zero_clone")])
NO_CLONE = np.array([K[n] for n in ("keep", "split", "split_transp", "split_child_big", "split_parent_big",
                                    "transp", "big_nograd", "nan_grad", "neg_large", "inf_large", "tie_g_in_large",
                                    "tie_g_out_small", "tie_s_eps")])
NO_KEPT_CHILD = np.array([K[n] for n in ("keep", "clone", "split_transp", "split_child_big", "tie_op_below_split",
                                         "transp")])
ALL_TRANSPARENT = np.array([K[n] for n in ("transp", "clone_transp", "split_transp", "tie_op_below",
                                           "tie_op_below_split")])


def empty_class_scene(which, N=2):
    P = 2 * BLOCK + 77
    if which == "no_split":
        return make_case(which, mix(P, 7, NO_SPLIT), N, 20.0)
    if which == "no_clone":
        return make_case(which, mix(P, 8, NO_CLONE), N, 20.0)
    if which == "no_kept_child":
        return make_case(which, mix(P, 9, NO_KEPT_CHILD), N, 20.0)
    if which == "nothing_by_opacity":
        return make_case(which, mix(P, 10, ALL_TRANSPARENT), N, 20.0)
    if which == "nothing_by_screen":
        return make_case(which, mix(P, 11), N, -1.0)
    raise KeyError(which)


EMPTY_CLASS = ("no_split", "no_clone", "no_kept_child", "nothing_by_opacity", "nothing_by_screen")
EMPTY_RESULT = ("nothing_by_opacity", "nothing_by_screen")


def edges_scene(N=2, screen=20.0, P=325):
    """Every kind and every tie, shuffled; the reference's own verdict on it is the fixture
    tests/golden/densify_edges_golden.npz."""
    k = np.resize(EVERY_KIND, P)
    np.random.default_rng(12).shuffle(k)
    return make_case("edges", k, N, screen)


def sized_scene(P, N=2, screen=20.0):
    """A mix of every kind at a given P (P = 1: one clone, see the module docstring's quirk)."""
    k = _filled(1, "clone") if P == 1 else mix(P, 100 + P, EVERY_KIND)
    return make_case(f"P{P}", k, N, screen)


def scan_pattern_kinds(P):
    """Kinds that differ from one classify block to the next in the way k_dens_scan walks them:
    thread t owns blocks [t * per, min(blocks, (t + 1) * per)).  Even threads: classes dense in the
    LAST block of the range (all clones, all splits or a mix, by t), none before it (all
    transparent).  Odd threads: the FIRST block all clones or all splits and mixes after it, so a
    base inside a range depends on the counts before it in the same range.  A thread left with a
    shorter range (the clipped tail) gets all-split blocks."""
    blocks = (P + BLOCK - 1) // BLOCK
    per = (blocks + SCAN_THREADS - 1) // SCAN_THREADS
    b = np.arange(blocks)
    t, i = b // per, b % per
    n_own = np.minimum(blocks, (t + 1) * per) - t * per
    # block pattern: 0 transparent, 1 clones, 2 splits, 3 mix
    pat = np.where(t % 2 == 0, np.where(i == n_own - 1, 1 + (t // 2) % 3, 0), np.where(i == 0, 1 + (t // 2) % 2, 3))
    pat = np.where(n_own < per, 2, pat)
    rowpat = np.repeat(pat, BLOCK)[:P]
    m = mix(P, 13)
    return np.select([rowpat == 0, rowpat == 1, rowpat == 2], [K["transp"], K["clone"], K["split"]], m)


def scan_scene(P, pattern, N=2, screen=20.0):
    k = scan_pattern_kinds(P) if pattern == "blocks" else mix(P, 14 + P, EVERY_KIND)
    return make_case(f"scan_{pattern}_P{P}", k, N, screen)


# ---------------------------------------------------------------- checks shared by the CPU and GPU tests

def assert_outputs_from_builder(case: Case, arrays: dict, model, groups_with_state=NAMES, step=2.0):
    """`model` (after densify_and_prune on `arrays`) has the builder's row count, and every copied
    tensor is the builder's gather of the input, bit for bit: all tensors except the children's xyz
    and scaling.  Moments: gathered on kept originals, zero on clone and child rows; step kept."""
    import torch

    from oracle import densify_oracle as DO

    dev = model._xyz.device
    src = torch.as_tensor(case.src_rows, device=dev)
    n_copy = int(case.totals[0] + case.totals[1])  # rows before the children
    for name, attr in zip(DO.NAMES, DO.ATTRS):
        got = getattr(model, attr).detach()
        want = torch.as_tensor(arrays[name], device=dev)[src]
        assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
        if name in ("xyz", "scaling"):
            got, want = got[:n_copy], want[:n_copy]
        assert torch.equal(got, want), name
        st = model.optimizer.state.get(getattr(model, attr))
        assert (st is not None) == (name in groups_with_state), name
        if st is None:
            continue
        assert float(st["step"]) == step
        for key in ("exp_avg", "exp_avg_sq"):
            mom = st[key]
            want = torch.as_tensor(arrays[f"{name}_{key}"], device=dev)[src]
            assert mom.shape == want.shape, (name, key)
            assert torch.equal(mom[:case.n_orig], want[:case.n_orig]), (name, key)
            assert not mom[case.n_orig:].any(), (name, key)
    for t in (model.xyz_gradient_accum, model.denom, model.max_radii2D):
        assert t.shape[0] == case.P_out and not t.any()
