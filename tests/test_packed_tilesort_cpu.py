"""The packed two-pass tile sort and its key-free ranges, restated in numpy (no GPU).

csrc/gs_forward.hip (tile_sort_packed_views) sorts the (tile, slot) instances of a two-pass grid as
one word per instance:

  pass 1  scatters by the low fb bits of the tile id into a padded layout: low digit l's region
          starts at the sum of the earlier digits' totals, each rounded up to the sort chunk, the
          gaps hold the drop key 0xFFFFFFFF, and the word is (tile >> fb) << sb | slot;
  pass 2  counts and scatters the padded words by their hb-bit high digit (drop on) and leaves
          word & (2^sb - 1) as the tile-sorted slot list;
  ranges  tile (h, l) owns base2[h] + [off2[h][blk0(l)], off2[h][blk0(l + 1)]) of that list, off2 the
          row-scanned [digit][block] histogram of pass 2, blk0(l) the first block of region l.

The restatement below follows those three steps block by block and is compared with
argsort(kind="stable") and searchsorted, for the digit splits of 13 .. 16 tile bits."""
import numpy as np
import pytest

DROP = np.uint32(0xFFFFFFFF)
SORT_TILE = 2048


def slot_bits(capacity):
    sb = 1
    while (1 << sb) <= capacity:
        sb += 1
    return sb  # capacity < 2^sb


def packed_sort(tile, capacity, fb, hb, tiles, chunk=SORT_TILE):
    """tile[n]: the tile id of every slot (n <= capacity).  Returns (point_list[n], ranges[tiles, 2])."""
    tile = np.asarray(tile, np.uint32)
    n = len(tile)
    sb = slot_bits(capacity)
    assert n <= capacity and hb + sb <= 32 and capacity >= chunk << fb
    # ---- pass 1: padded regions by low digit ----
    low = tile & np.uint32((1 << fb) - 1)
    totals = np.bincount(low, minlength=1 << fb).astype(np.int64)
    padded = (totals + chunk - 1) // chunk * chunk
    start = np.concatenate([[0], np.cumsum(padded)])
    n2 = int(start[-1])
    assert n2 <= capacity + (chunk << fb)
    blk0 = start // chunk  # first block of region l; blk0[2^fb]: the end
    buf = np.full(n2, DROP, np.uint32)
    for l in range(1 << fb):
        idx = np.nonzero(low == l)[0]  # slot order: the scatter is stable
        buf[start[l]:start[l] + len(idx)] = ((tile[idx] >> np.uint32(fb)) << np.uint32(sb)) | idx.astype(np.uint32)
    assert int((buf == DROP).sum()) == n2 - n  # only the gaps hold the drop key
    # ---- pass 2: [digit][block] histogram, row scan, scatter ----
    nb2 = (capacity + (chunk << fb) + chunk - 1) // chunk
    keep = buf != DROP
    digit = (buf >> np.uint32(sb)) & np.uint32((1 << hb) - 1)
    block = np.arange(n2) // chunk
    hist = np.zeros((1 << hb, nb2), np.int64)
    np.add.at(hist, (digit[keep], block[keep]), 1)
    row_total = hist.sum(1)
    off2 = np.cumsum(hist, 1) - hist
    base2 = np.cumsum(row_total) - row_total
    out = np.full(n, DROP, np.uint32)
    for b in range(int(blk0[-1])):
        w = buf[b * chunk:(b + 1) * chunk]
        w = w[w != DROP]
        d = (w >> np.uint32(sb)) & np.uint32((1 << hb) - 1)
        for h in np.unique(d):
            run = w[d == h]
            p = base2[h] + off2[h, b]
            out[p:p + len(run)] = run & np.uint32((1 << sb) - 1)
    # ---- ranges from the offsets ----
    ranges = np.zeros((tiles, 2), np.uint32)
    for t in range(tiles):
        h, l = t >> fb, t & ((1 << fb) - 1)
        x = off2[h, blk0[l]] if blk0[l] < nb2 else row_total[h]
        y = off2[h, blk0[l + 1]] if blk0[l + 1] < nb2 else row_total[h]
        if x < y:
            ranges[t] = (base2[h] + x, base2[h] + y)
    return out, ranges


def reference(tile, tiles):
    tile = np.asarray(tile, np.int64)
    order = np.argsort(tile, kind="stable")
    s = tile[order]
    lo, hi = np.searchsorted(s, np.arange(tiles), "left"), np.searchsorted(s, np.arange(tiles), "right")
    ranges = np.stack([lo, hi], 1).astype(np.uint32)
    ranges[lo == hi] = 0
    return order.astype(np.uint32), ranges


def region_scene(fb, hb, tiles, rng):
    """Low-digit totals of 0, 1, 2047, 2048 and 2049 (and a few random ones), each spread over the
    high digits that exist below `tiles`; slot order shuffled."""
    totals = {0: 2048, 1: 2049, 2: 2047, 3: 1, 5: 0, (1 << fb) - 1: 4097, (1 << fb) - 2: 300}
    out = []
    for l, cnt in totals.items():
        highs = np.arange(((tiles - 1 - l) >> fb) + 1)  # h with (h << fb | l) < tiles
        out.append((rng.choice(highs, cnt) << fb) | l)
    t = np.concatenate(out).astype(np.uint32)
    rng.shuffle(t)
    return t


SPLITS = [(6, 7, 8160), (7, 7, 129 * 64), (7, 8, 129 * 128), (8, 8, 65536)]


@pytest.mark.parametrize("fb,hb,tiles", SPLITS)
def test_region_totals_on_and_around_the_sort_tile(fb, hb, tiles):
    rng = np.random.default_rng(fb * 100 + hb)
    tile = region_scene(fb, hb, tiles, rng)
    cap = max(len(tile), SORT_TILE << fb)
    got = packed_sort(tile, cap, fb, hb, tiles)
    want = reference(tile, tiles)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize("fb,hb,tiles", SPLITS)
def test_count_below_the_capacity_and_one_digit_only(fb, hb, tiles):
    rng = np.random.default_rng(7)
    cap = 3 * (SORT_TILE << fb) + 77  # the count is far below it: the last blocks are empty
    # one non-empty low digit only, in several high digits (the last region ends the padded list)
    for l in (0, 3, (1 << fb) - 1):
        highs = np.arange(((tiles - 1 - l) >> fb) + 1)
        tile = ((rng.choice(highs, 5000) << fb) | l).astype(np.uint32)
        got = packed_sort(tile, cap, fb, hb, tiles)
        want = reference(tile, tiles)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
    # no instance at all
    got = packed_sort(np.zeros(0, np.uint32), cap, fb, hb, tiles)
    assert len(got[0]) == 0 and not got[1].any()


@pytest.mark.parametrize("fb,hb,tiles", SPLITS)
def test_tile_ids_at_and_past_the_grid(fb, hb, tiles):
    """Ids in [tiles, 2^(fb + hb)) sort like any other (the list stays a stable sort of all the
    slots) and get no range: the ranges array has `tiles` rows."""
    rng = np.random.default_rng(11)
    top = 1 << (fb + hb)
    tile = rng.integers(0, tiles, 20000).astype(np.uint32)
    tile[::7] = tiles - 1
    if top > tiles:
        tile[1::7] = tiles
        tile[2::7] = top - 1
    cap = max(len(tile), SORT_TILE << fb)
    got = packed_sort(tile, cap, fb, hb, tiles)
    want = reference(tile, tiles)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_larger_sort_chunks():
    """Above 4096 sort blocks a block walks several 2048-key tiles: the regions are padded to that
    chunk, so that they still start on a block of the second pass."""
    rng = np.random.default_rng(3)
    fb, hb, tiles = 6, 7, 8160
    tile = region_scene(fb, hb, tiles, rng)
    got = packed_sort(tile, 3 * SORT_TILE << fb, fb, hb, tiles, chunk=3 * SORT_TILE)
    want = reference(tile, tiles)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
