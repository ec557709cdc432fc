"""CPU checks of the constructed scenes (tests/constructed_scenes.py) against the oracle.

For every scene the GPU tests use: the counts the builder promises (computed from the construction
alone) equal what oracle.forward(..., intermediates=True) gives -- num_rendered, tiles_touched, depth
bits, ranges, the whole ordered list, the owners' record runs, the promised tiles' largest
n_contrib -- and the property the scene exists for is present.  These are conditions on the inputs:
exact, no tolerance, nothing taken from the HIP library."""
import numpy as np
import pytest

import constructed_scenes as cs_mod
from constructed_scenes import DUP_SLOTS, LB_MAX_P, ROUND, SORT_TILE, TILE, cached, oracle_forward

SPECS = cs_mod.all_scene_specs()


def _tile_max(n_contrib, gx, gy):
    """Largest n_contrib of every tile (the ragged last column / row padded with 0)."""
    H, W = n_contrib.shape
    full = np.zeros((gy * TILE, gx * TILE), np.int64)
    full[:H, :W] = n_contrib
    return full.reshape(gy, TILE, gx, TILE).max(axis=(1, 3)).reshape(-1)


def _owner_layout(fw):
    """Owners in (depth bits, index) order and their record offsets, from the oracle's outputs."""
    touched = fw["tiles_touched"].astype(np.int64)
    vis = np.nonzero(touched > 0)[0]
    bits = fw["depth"].view(np.uint32)
    order = vis[np.lexsort((vis, bits[vis]))]
    return order, np.concatenate([[0], np.cumsum(touched[order])])


def _check_promises(cs, fw):
    assert fw["num_rendered"] == cs.I
    np.testing.assert_array_equal(fw["tiles_touched"], cs.tiles_touched)
    assert int((fw["tiles_touched"] > 0).sum()) == cs.V
    seen = fw["radii"] > 0
    assert seen[cs.tiles_touched > 0].all()
    np.testing.assert_array_equal(fw["depth"].view(np.uint32)[seen], cs.depth_bits[seen])
    np.testing.assert_array_equal(fw["ranges"], cs.ranges)
    np.testing.assert_array_equal(fw["ranges"][:, 1].astype(np.int64) - fw["ranges"][:, 0], cs.list_len)
    np.testing.assert_array_equal(fw["point_list"], cs.point_list)
    order, offsets = _owner_layout(fw)
    np.testing.assert_array_equal(order, cs.sorted_gid)
    np.testing.assert_array_equal(offsets, cs.offsets)
    gx, gy = cs_mod.grid(cs.cam.image_width, cs.cam.image_height)
    tmax = _tile_max(fw["n_contrib"], gx, gy)
    assert (tmax <= cs.list_len).all()
    for t, n in cs.n_eff.items():
        assert tmax[t] == n, (cs.name, t, int(tmax[t]), n)
    return tmax


@pytest.mark.parametrize("fn,args", [s[1:] for s in SPECS], ids=[s[0] for s in SPECS])
def test_promised_counts_hold(oracle, fn, args):
    cs = cached(fn, *args)
    fw = oracle_forward(oracle, cs)
    _check_promises(cs, fw)
    # absent Gaussians: none has an instance; the faint ones keep a radius, those behind have none
    ab, behind = cs.props["absent"], cs.props["behind"]
    assert (fw["tiles_touched"][ab] == 0).all() and (fw["radii"][behind] == 0).all()
    faint = np.setdiff1d(ab, behind)
    assert (fw["radii"][faint] > 0).all()
    if len(ab) >= 20:  # depth rank != index
        assert not np.array_equal(cs.sorted_gid, np.arange(cs.V))


@pytest.mark.parametrize("N", cs_mod.EXACT_SIZES)
def test_exact_sizes_are_exact(oracle, N):
    cs = cached(cs_mod.exact_size, N)
    fw = oracle_forward(oracle, cs)
    assert fw["num_rendered"] == N and int((fw["tiles_touched"] > 0).sum()) == N
    assert len(cs.props["absent"]) == N // 3
    _, offsets = _owner_layout(fw)
    # every owner has one record: a duplicate block of I >= 2048 is 2048 one-slot segments, a
    # record-sum chunk 64 one-record owners
    np.testing.assert_array_equal(offsets, np.arange(N + 1))
    if N >= 3:  # ties: fewer distinct depths than Gaussians in some tile, all three values present
        assert len(np.unique(fw["depth"][fw["tiles_touched"] > 0])) == min(3, -(-N // 104))


@pytest.mark.parametrize("P", cs_mod.EXACT_TOTALS)
def test_exact_totals(oracle, P):
    cs = cached(cs_mod.exact_total, P)
    fw = oracle_forward(oracle, cs)
    assert len(fw["radii"]) == P and fw["num_rendered"] == P - P // 4 == int((fw["tiles_touched"] > 0).sum())


def test_range_edge_on_a_ranges_workgroup_edge(oracle):
    cs = cached(cs_mod.exact_size, 2048, 256, 256)
    fw = oracle_forward(oracle, cs)
    assert (fw["ranges"][:, 1] - fw["ranges"][:, 0] == 8).all()
    assert cs_mod.RANGES_WG in fw["ranges"][:, 0]  # a range starts on instance 1024


@pytest.mark.parametrize("W,H,bits", [(203, 117, 7), (256, 256, 8), (272, 256, 9)])
def test_one_per_tile(oracle, W, H, bits):
    cs = cached(cs_mod.one_per_tile, W, H)
    fw = oracle_forward(oracle, cs)
    tiles = len(cs.list_len)
    assert fw["num_rendered"] == tiles and (fw["ranges"][:, 1] - fw["ranges"][:, 0] == 1).all()
    assert (tiles - 1).bit_length() == bits  # 8 bits: one tile-sort pass; 9: two
    assert len(np.unique(fw["depth"][fw["tiles_touched"] > 0])) == 1


PLANS = {14: [7, 7], 15: [7, 8], 16: [8, 8], 17: [5, 6, 6]}  # tile bits -> digit widths, first pass first


@pytest.mark.parametrize("W,H,bits", cs_mod.LARGE_GRIDS)
def test_large_grids_reach_the_later_pass_plans(W, H, bits):
    """The grids above 1080p: the bit count of the tile ids and the tile sort's digit plan it
    selects, restated here in plain Python (nothing imported from the library).  An odd number of
    passes leaves the sorted list in the second ping-pong buffer: one pass (<= 8 bits) and the
    three passes of 17 bits.  The promises themselves are checked by test_promised_counts_hold."""
    cs = cached(cs_mod.one_per_tile, W, H)
    gx, gy = cs_mod.grid(W, H)
    tiles = gx * gy
    assert len(cs.list_len) == tiles and cs.I == cs.V == tiles and (cs.list_len == 1).all()
    assert (tiles - 1).bit_length() == bits
    assert len(np.unique(cs.depth_bits[cs.tiles_touched > 0])) == 1
    plan = cs_mod.tile_sort_plan(tiles)
    assert plan == PLANS[bits] and sum(plan) == bits and max(plan) <= 8
    assert (len(plan) % 2 == 1) == (bits == 17)
    assert {(203, 117): [7], (256, 256): [8], (272, 256): [4, 5], (1920, 1080): [6, 7]} == {
        wh: cs_mod.tile_sort_plan(cs_mod.grid(*wh)[0] * cs_mod.grid(*wh)[1])
        for wh in ((203, 117), (256, 256), (272, 256), (1920, 1080))}
    if (W, H) == (4096, 4096):
        assert tiles == 1 << 16 and W % TILE == 0 and H % TILE == 0  # the last two-pass size, no ragged edge
    if (W, H) == cs_mod.GRID17:
        assert (gx, gy, tiles) == (257, 256, 65792) and W % TILE and H % TILE


def test_seventeen_bit_scenes():
    """What the three 17-bit scenes besides one_per_tile exist for (facts of the construction)."""
    tiles = 65792
    t = cached(cs_mod.tie_clones, 40000, *cs_mod.GRID17)
    assert t.I == t.V == t.P == 80000 and len(np.unique(t.depth_bits)) == 1
    # a clone pair in each of the first 40,000 tiles: tile ids that differ in all three digits
    assert (t.list_len[:40000] == 2).all() and not t.list_len[40000:].any() and 40000 > 1 << (5 + 6)
    assert np.array_equal(t.point_list[:2], [0, 40000])    # the tie resolves by index
    f = cached(cs_mod.few_big)
    assert (f.P, f.I, f.V) == (12, 197381, 8) and f.I == 3 * tiles + 5
    assert f.I > DUP_SLOTS * f.P                           # unbalanced: the per-splat duplicate
    big = f.props["big"]
    assert (f.tiles_touched[big] == tiles).all() and tiles > 65535
    assert sorted(f.list_len[list(cs_mod.FEW_BIG_TILES)]) == [4] * 5 and (f.list_len >= 3).all()
    assert f.sorted_gid[0] == big[0] and len(np.unique(f.depth_bits[f.sorted_gid[1:]])) == 1
    assert len(f.props["absent"]) == 4
    o = cached(cs_mod.owner_among_many)
    assert (o.P, o.I, o.V) == (66793, 131584, tiles + 1) and o.I <= DUP_SLOTS * o.P  # balanced: k_duplicate_lb
    a, b = o.run(o.props["big"][0])
    assert b - a == tiles and (b - 1) // DUP_SLOTS - a // DUP_SLOTS + 1 == 33  # 33 duplicate blocks
    assert (o.list_len == 2).all() and len(np.unique(o.depth_bits[o.tiles_touched > 0])) == 3
    assert len(o.props["absent"]) == 1000


def test_tie_clones_span_sort_tiles_and_decide_the_image(oracle):
    cs = cached(cs_mod.tie_clones)
    fw = oracle_forward(oracle, cs)
    tied = np.nonzero(fw["tiles_touched"] > 0)[0]
    assert len(tied) >= 5000 and len(np.unique(fw["depth"].view(np.uint32)[tied])) == 1
    assert len(np.unique(tied // SORT_TILE)) >= 3            # depth sort: keys in index order
    assert len(np.unique(np.arange(fw["num_rendered"]) // SORT_TILE)) >= 3  # tile sort: one key per slot
    n = cs.props["n_pairs"]
    m = cs.scene.means3D.numpy()
    assert np.array_equal(m[:n], m[n:]) and not np.array_equal(cs.scene.shs.numpy()[:n], cs.scene.shs.numpy()[n:])
    # not vacuous: the other tie order gives another image
    rev = oracle.forward(cs_mod.oracle_scene(oracle, cs.cam, cs_mod.reversed_scene(cs), cs.bg))
    assert not np.array_equal(rev["color"], fw["color"])
    assert np.abs(rev["color"] - fw["color"]).max() > 0.05


def test_digit_extremes_fill_the_end_bins(oracle):
    cs = cached(cs_mod.digit_extremes)
    fw = oracle_forward(oracle, cs)
    vis = fw["tiles_touched"] > 0
    bits = fw["depth"].view(np.uint32)[vis]
    for shift in (0, 8, 16):
        assert set(np.unique((bits >> shift) & 255)) == set(cs_mod.DIGIT_BYTES)
    z = fw["depth"][vis]
    assert z.min() > 0.2 and z.max() < 100.0
    assert len(np.unique(bits)) * 2 == len(bits)  # every pattern twice


@pytest.mark.parametrize("L", cs_mod.HOT_LENGTHS)
def test_hot_tile_list_and_n_eff(oracle, L):
    cs = cached(cs_mod.hot_tile, L)
    fw = oracle_forward(oracle, cs)
    gx, gy = cs_mod.grid(cs_mod.HOT_W, cs_mod.HOT_H)
    tmax = _tile_max(fw["n_contrib"], gx, gy)
    assert tmax[cs_mod.HOT_TILE] == L and tmax.sum() == L
    np.testing.assert_array_equal(fw["ranges"][cs_mod.HOT_TILE], (0, L))  # one range over the whole list
    assert fw["final_T"].min() >= 0.09


def test_two_hot_tiles(oracle):
    cs = cached(cs_mod.hot_tile, 257, True)
    fw = oracle_forward(oracle, cs)
    gx, gy = cs_mod.grid(cs_mod.HOT_W, cs_mod.HOT_H)
    tmax = _tile_max(fw["n_contrib"], gx, gy)
    assert cs.props["hot"] == [cs_mod.HOT_TILE, gx * gy - 1]
    assert tmax[cs_mod.HOT_TILE] == 257 and tmax[-1] == 257 and tmax.sum() == 514


STOPS = [(n, "single") for n in cs_mod.STOP_N_EFF] + [(65, "tail_here"), (129, "tail_elsewhere")]


@pytest.mark.parametrize("n_eff,variant", STOPS)
def test_stop_lands_on_the_promised_entry(oracle, n_eff, variant):
    cs = cached(cs_mod.stop_edge, n_eff, variant)
    fw = oracle_forward(oracle, cs)
    W, H = cs.cam.image_width, cs.cam.image_height
    gx, gy = cs_mod.grid(W, H)
    hot, tail_tile = cs.props["hot"], cs.props["tail_tile"]
    ty, tx = divmod(hot, gx)
    nc = fw["n_contrib"][TILE * ty:TILE * ty + TILE, TILE * tx:TILE * tx + TILE]
    assert nc.max() == n_eff and nc.min() == n_eff - 1
    assert cs.list_len[tail_tile] >= 2 * n_eff if variant != "tail_elsewhere" else cs.list_len[tail_tile] >= n_eff
    cut, cut_max = cs.tile_cuts(fw["n_contrib"])
    # records past the cut: at least one whole 64-record chunk, whatever the chunk base
    assert cs.I - cut_max >= 2 * ROUND
    # no tail instance is walked by its tile
    slots = cs.slot_of_list()
    a, b = cs.ranges[tail_tile]
    tail_slots = slots[a:b][-cs.props["n_tail"]:]
    assert tail_slots.min() >= cut[tail_tile] and tail_slots.min() >= cut_max
    if variant == "single":
        assert int(np.argmax(cut)) == hot == tail_tile
    if variant == "tail_elsewhere":
        assert tail_tile != hot and cut[tail_tile] < cut_max and int(np.argmax(cut)) != tail_tile


def test_big_owner_runs(oracle):
    s = cached(cs_mod.big_owner, "straddle")
    fw = oracle_forward(oracle, s)
    order, offsets = _owner_layout(fw)
    g = s.props["big"][0]
    assert fw["tiles_touched"][g] == 300
    r = int(np.nonzero(order == g)[0][0])
    a, b = int(offsets[r]), int(offsets[r + 1])
    assert a < DUP_SLOTS < b and (DUP_SLOTS - a) % 20 != 0  # slot 2048 inside a row segment
    assert (a, b) == s.run(g) == (1898, 2198)

    c = cached(cs_mod.big_owner, "chunk_start")
    fw = oracle_forward(oracle, c)
    order, offsets = _owner_layout(fw)
    g = c.props["big"][1]
    r = int(np.nonzero(order == g)[0][0])
    a, b = int(offsets[r]), int(offsets[r + 1])
    wave_base = int(offsets[ROUND * (r // ROUND)])
    assert r % ROUND != 0 and a % ROUND == 0 and (a - wave_base) % ROUND == 0 and a > wave_base
    assert b - a == 300 and (b - 1) // ROUND - a // ROUND == 4  # the owner spans five chunks

    p = cached(cs_mod.big_owner, "pair")
    fw = oracle_forward(oracle, p)
    g0, g1 = p.props["big"]
    assert fw["tiles_touched"][g0] == 300 and fw["tiles_touched"][g1] == 300
    bits = fw["depth"].view(np.uint32)
    assert bits[g0] == bits[g1] and int((bits[fw["tiles_touched"] > 0] == bits[g0]).sum()) == 302
    assert (p.list_len == 3).all()


@pytest.mark.parametrize("P,lookback", [(LB_MAX_P, True), (LB_MAX_P + 1, False)])
def test_path_switch_sizes(oracle, P, lookback):
    cs = cached(cs_mod.path_switch, P)
    fw = oracle_forward(oracle, cs)
    assert cs.P == P == (1_048_576 if lookback else 1_048_577)
    assert ((P + 2047) // 2048 <= 512) == lookback
    assert fw["num_rendered"] == SORT_TILE + 1 and int((fw["radii"] > 0).sum()) == SORT_TILE + 1
    vis = np.nonzero(fw["tiles_touched"])[0]
    assert vis.min() < P // 100 and vis.max() > P - P // 100  # scattered through the index range
    assert len(np.unique(fw["depth"][vis])) == 3


def test_two_views_counts_differ(oracle):
    cs, cam_b, pb = cached(cs_mod.two_views)
    fa = oracle_forward(oracle, cs)
    _check_promises(cs, fa)
    assert fa["num_rendered"] == SORT_TILE + 1
    fb = oracle.forward(cs_mod.oracle_scene(oracle, cam_b, cs.scene, cs.bg), intermediates=True)
    assert fb["num_rendered"] == pb["I"] == SORT_TILE
    np.testing.assert_array_equal(fb["tiles_touched"], pb["tiles_touched"])
    np.testing.assert_array_equal(fb["ranges"], pb["ranges"])
    np.testing.assert_array_equal(fb["point_list"], pb["point_list"])
    lone = cs.props["lone"]
    assert fa["tiles_touched"][lone] == 1 and fb["tiles_touched"][lone] == 0
