"""Scenes whose instance counts are exact by construction (CPU only, seeded).

Every other parity scene is drawn by gs_scenes.random_gaussians, so the instance count I, the count
V of Gaussians with instances, the per-tile list lengths and the per-Gaussian record runs are
whatever the seed gives.  The scenes here put those counts on the sizes where the ordering and
binning kernels change behaviour (sort tile 2048, scan tile 2048 / 1024, duplicate block 2048,
4 x 256 instances per k_ranges workgroup, 64 staged entries per render round, 64 records per
record-sum chunk) and make depth ties, which random depths never produce.

Building block: the one-tile Gaussian under gs_scenes.identity_camera(W, H).  It is isotropic with
a screen sigma of 1 px (scale = sigma z / fx), its mean projects to the centre (16 tx + 7.5,
16 ty + 7.5) of a chosen tile, and its depth z is chosen freely (also as a uint32 bit pattern: the
identity view matrix makes the view depth exactly z).  The 2D covariance is
sigma^2 (1 + |t|^2 / z^2) + 0.3 <= 3.3 at most for tan^2(fovx / 2) + tan^2(fovy / 2) <= 2 (asserted), the
radius ceil(3 sqrt(.)) <= 6 px, within the 7.5 px from the tile centre to the tile's edges, so the
tile rectangle, and the tile-exact row span inside it, is that single tile: one instance.
Opacities are >= 0.01, so the pixel next to the centre (q ~ 0.4) lies inside the alpha >= 1/255
ellipse (q <= 2 ln(2.55) = 1.87) and the span is not empty.

Other kinds:
  - "all-tiles" Gaussians (full-screen: sigma 2000 px, faint; cover: sigma 40 px, opacity 0.999):
    one instance in every tile of the grid.  The builder checks in fp64 that the rectangle
    (radius >= 3 sigma) reaches every tile from the mean and that the farthest pixel of the image
    has q <= d^2 / sigma^2 below half the culling limit 2 ln(255 opacity): the row spans are
    conservative, so a tile holding such a pixel is listed.
  - "absent" Gaussians, interleaved by index so that depth rank != index: behind the camera
    (radius 0), or opacity 0.002 < 1/255 (radius > 0 but no instance: its depth key is the
    dropped one of the first depth-sort pass).

A Constructed carries the scene and what it promises, all computed here in numpy from the
construction alone (never from the oracle or the HIP library): tiles_touched, depth bits, I, V, the
per-tile list lengths, ranges, the whole (tile, depth bits, index)-ordered list, the depth-ordered
owners with their record runs [offsets[r], offsets[r + 1]) and, where the scene controls it, a
tile's n_eff (its largest n_contrib).  tests/test_constructed_scenes.py checks every promise
against the oracle; tests/test_gpu_constructed.py runs the HIP path on the same scenes.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

import gs_scenes

TILE = 16
SORT_TILE = 2048   # keys per radix-sort tile (gs_sortscan.h SORT_TILE) = look-back scan tile (LB_TILE)
DUP_SLOTS = 2048   # instance slots per k_duplicate_lb workgroup
SCAN_TILE = 1024   # elements per tile of the 3-launch scan (k_scan_reduce / k_scan_down)
RANGES_WG = 1024   # instances per k_ranges workgroup (4 per lane)
ROUND = 64         # entries staged per render round; records per record-sum chunk; ranks per wave
LB_MAX_P = 512 * 2048  # the last P of the look-back ordering path (lb_tiles(P) <= LB_STATIC_MAX)

FAINT = 0.01       # opacity of a "faint" one-tile Gaussian: alpha 0.00825 at its 4 centre pixels
ABSENT_OPACITY = 0.002  # < 1/255: no pixel reaches the alpha threshold


def f32_bits(z):
    return np.asarray(z, np.float32).view(np.uint32)


def bits_f32(b):
    return np.asarray(b, np.uint32).view(np.float32)


def grid(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


@dataclass
class Constructed:
    name: str
    cam: gs_scenes.MiniCamera
    scene: gs_scenes.GaussianScene
    bg: np.ndarray
    tiles_touched: np.ndarray   # [P] uint32
    depth_bits: np.ndarray      # [P] uint32 (view depth of the mean)
    I: int
    V: int
    list_len: np.ndarray        # [tiles]
    ranges: np.ndarray          # [tiles, 2] uint32, (0, 0) for an empty tile
    point_list: np.ndarray      # [I] Gaussian index, ordered by (tile, depth bits, index)
    sorted_gid: np.ndarray      # [V] owners in (depth bits, index) order
    offsets: np.ndarray         # [V + 1] first record slot of each owner, offsets[V] = I
    n_eff: dict = field(default_factory=dict)   # tile -> promised largest n_contrib
    props: dict = field(default_factory=dict)   # scene-specific facts (indices, tiles) for the tests

    @property
    def P(self):
        return self.scene.P

    def rank_of(self, gid):
        return int(np.nonzero(self.sorted_gid == gid)[0][0])

    def run(self, gid):
        """[start, end) record slots of Gaussian gid."""
        r = self.rank_of(gid)
        return int(self.offsets[r]), int(self.offsets[r + 1])

    def slot_of_list(self):
        """Record slot of every entry of point_list.  An owner's records follow its tiles row by
        row (k_duplicate_lb), i.e. in tile order for the one-tile and all-tiles kinds here."""
        V = len(self.sorted_gid)
        rank = np.full(self.P, -1, np.int64)
        rank[self.sorted_gid] = np.arange(V)
        tiles = len(self.list_len)
        tile_of = np.repeat(np.arange(tiles), self.list_len)
        g = self.point_list.astype(np.int64)
        within = np.where(self.tiles_touched[g] == 1, 0, tile_of)
        return self.offsets[rank[g]] + within

    def tile_cuts(self, n_contrib):
        """(tile_cut[tiles], cut_max) as k_tile_order computes them from a forward's n_contrib:
        1 + the slot of the last instance a tile's walk reaches (0: none)."""
        W, H = self.cam.image_width, self.cam.image_height
        gx, gy = grid(W, H)
        slots = self.slot_of_list()
        cut = np.zeros(gx * gy, np.int64)
        for t in range(gx * gy):
            ty, tx = divmod(t, gx)
            n = int(n_contrib[TILE * ty:TILE * ty + TILE, TILE * tx:TILE * tx + TILE].max(initial=0))
            n = min(n, int(self.list_len[t]))
            if n:
                cut[t] = slots[int(self.ranges[t, 0]) + n - 1] + 1
        return cut, int(cut.max(initial=0))


def promises(P, tiles, one_tile, all_tiles, depth_bits):
    """The ordering facts of a scene whose Gaussian i has one instance in tile one_tile[i] (>= 0),
    one in every tile (all_tiles[i]) or none."""
    one_tile = np.asarray(one_tile, np.int64)
    all_tiles = np.asarray(all_tiles, bool)
    bits = np.asarray(depth_bits, np.uint32)
    touched = np.where(all_tiles, tiles, (one_tile >= 0).astype(np.int64)).astype(np.uint32)
    g1 = np.nonzero((one_tile >= 0) & ~all_tiles)[0]
    ga = np.nonzero(all_tiles)[0]
    inst_gid = np.concatenate([g1, np.repeat(ga, tiles)])
    inst_tile = np.concatenate([one_tile[g1], np.tile(np.arange(tiles), len(ga))])
    o = np.lexsort((inst_gid, bits[inst_gid], inst_tile))
    point_list = inst_gid[o].astype(np.uint32)
    list_len = np.bincount(inst_tile, minlength=tiles).astype(np.int64)
    end = np.cumsum(list_len)
    ranges = np.stack([end - list_len, end], 1)
    ranges[list_len == 0] = 0
    vis = np.nonzero(touched > 0)[0]
    sorted_gid = vis[np.lexsort((vis, bits[vis]))]
    offsets = np.concatenate([[0], np.cumsum(touched[sorted_gid].astype(np.int64))])
    return dict(tiles_touched=touched, depth_bits=bits, I=int(len(inst_gid)), V=int(len(vis)), list_len=list_len,
                ranges=ranges.astype(np.uint32), point_list=point_list, sorted_gid=sorted_gid, offsets=offsets)


class Builder:
    """Collects Gaussians of the kinds above for identity_camera(W, H); build() fixes the index
    order (optionally a seeded permutation, with absent Gaussians interleaved) and returns the
    scene with its promises."""

    def __init__(self, W, H, seed=0, bg=(0.0, 0.0, 0.0)):
        self.W, self.H = W, H
        self.gx, self.gy = grid(W, H)
        self.tiles = self.gx * self.gy
        self.cam = gs_scenes.identity_camera(W, H)
        self.tanx, self.tany = math.tan(self.cam.FoVx / 2), math.tan(self.cam.FoVy / 2)
        assert self.tanx ** 2 + self.tany ** 2 <= 2.0
        self.fx = W / (2.0 * self.tanx)
        self.rng = np.random.default_rng(seed)
        self.bg = np.asarray(bg, np.float32)
        # per Gaussian: pixel position, depth bits, sigma (px), opacity, colour, one_tile, all_tiles
        self.px, self.py, self.bits, self.sigma, self.op, self.col, self.one, self.all = ([] for _ in range(8))

    def tile_centre(self, tile):
        ty, tx = divmod(int(tile), self.gx)
        return TILE * tx + 7.5, TILE * ty + 7.5

    def _add(self, px, py, bits, sigma, op, col, one, al):
        z = float(bits_f32(bits))
        assert 0.2 < z < 100.0, z
        self.px.append(px), self.py.append(py), self.bits.append(np.uint32(bits)), self.sigma.append(sigma)
        self.op.append(op), self.col.append(col), self.one.append(one), self.all.append(al)
        return len(self.px) - 1

    def _depth(self, depth, depth_bits):
        return np.uint32(depth_bits) if depth_bits is not None else f32_bits(depth)[()]

    def add_tile(self, tile, depth=None, opacity=FAINT, colour=None, depth_bits=None):
        """One-tile Gaussian in `tile` at view depth `depth` (or the float with bits depth_bits)."""
        assert 0 <= tile < self.tiles and 0.01 <= opacity <= 1.0
        px, py = self.tile_centre(tile)
        col = self.rng.random(3) if colour is None else colour
        return self._add(px, py, self._depth(depth, depth_bits), 1.0, opacity, col, int(tile), False)

    def add_all_tiles(self, depth, opacity, colour=None, sigma_px=2000.0, tile=None, depth_bits=None):
        """A Gaussian with one instance in every tile, centred on the image (or on `tile`)."""
        px, py = ((self.W - 1) / 2.0, (self.H - 1) / 2.0) if tile is None else self.tile_centre(tile)
        # the rectangle: radius >= 3 sigma reaches every tile column / row from the mean
        assert 3.0 * sigma_px >= max(px, self.W - px, py, self.H - py) + TILE
        # the span: the farthest pixel has q <= d^2 / sigma^2 (cov2D >= sigma^2 I), below half the limit
        d2 = max(px, self.W - 1 - px) ** 2 + max(py, self.H - 1 - py) ** 2
        assert d2 / sigma_px ** 2 <= 0.5 * 2.0 * math.log(255.0 * opacity), (d2, sigma_px, opacity)
        col = self.rng.random(3) if colour is None else colour
        return self._add(px, py, self._depth(depth, depth_bits), sigma_px, opacity, col, -1, True)

    def add_cover(self, tile, depth, colour=None):
        """Opaque over `tile` and its neighbours (alpha clamps to 0.99 within 5 px of the centre)."""
        return self.add_all_tiles(depth, 0.999, colour, sigma_px=40.0, tile=tile)

    def build(self, name, shuffle=False, n_absent=0, absent_kinds=("behind", "faint"), n_eff=None, props=None):
        n = len(self.px)
        P = n + n_absent
        rng = self.rng
        src = rng.permutation(n) if shuffle else np.arange(n)
        # positions of the real Gaussians in the final index order: a sorted random subset
        pos = np.sort(rng.choice(P, n, replace=False)) if n_absent else np.arange(n)
        index_of = np.empty(n, np.int64)  # builder handle -> final index
        index_of[src] = pos
        px = np.full(P, 7.5)
        py = np.full(P, 7.5)
        z = np.full(P, 3.0, np.float32)
        sigma = np.ones(P)
        op = np.full(P, ABSENT_OPACITY, np.float32)
        col = rng.random((P, 3))
        one = np.full(P, -1, np.int64)
        al = np.zeros(P, bool)
        if n:
            px[pos], py[pos] = np.asarray(self.px)[src], np.asarray(self.py)[src]
            z[pos] = bits_f32(np.asarray(self.bits, np.uint32)[src])
            sigma[pos] = np.asarray(self.sigma)[src]
            op[pos] = np.asarray(self.op, np.float32)[src]
            col[pos] = np.asarray(self.col)[src]
            one[pos], al[pos] = np.asarray(self.one)[src], np.asarray(self.all)[src]
        absent = np.ones(P, bool)
        absent[pos] = False
        a_idx = np.nonzero(absent)[0]
        if len(a_idx):
            # absent Gaussians sit on tile centres too (a faint one has a radius and a rectangle)
            t = rng.integers(0, self.tiles, len(a_idx))
            px[a_idx], py[a_idx] = TILE * (t % self.gx) + 7.5, TILE * (t // self.gx) + 7.5
            z[a_idx] = rng.choice(np.array([2.0, 3.0, 5.0], np.float32), len(a_idx))
        behind = np.zeros(P, bool)
        if len(a_idx):
            kind = np.arange(len(a_idx)) % len(absent_kinds)
            behind[a_idx[np.asarray(absent_kinds)[kind] == "behind"]] = True
        z64 = z.astype(np.float64)
        x = ((2.0 * px + 1.0) / self.W - 1.0) * self.tanx * z64
        y = ((2.0 * py + 1.0) / self.H - 1.0) * self.tany * z64
        zs = np.where(behind, -z64, z64)
        means = np.stack([np.where(behind, -x, x), np.where(behind, -y, y), zs], 1).astype(np.float32)
        assert np.array_equal(means[~behind, 2], z[~behind])  # the depth bits survive
        scales = np.repeat((sigma * z64 / self.fx)[:, None], 3, 1).astype(np.float32)
        rots = np.zeros((P, 4), np.float32)
        rots[:, 0] = 1.0
        shs = ((col - 0.5) / gs_scenes.SH_C0).astype(np.float32)[:, None, :]
        sc = gs_scenes.GaussianScene(torch.from_numpy(means), torch.from_numpy(op[:, None].copy()),
                                     torch.from_numpy(scales), torch.from_numpy(rots),
                                     torch.from_numpy(np.ascontiguousarray(shs)), 0)
        pr = promises(P, self.tiles, one, al, f32_bits(z))
        props = dict(props or {})
        props["index_of"] = index_of
        props["absent"] = a_idx
        props["behind"] = np.nonzero(behind)[0]
        return Constructed(name=name, cam=self.cam, scene=sc, bg=self.bg, n_eff=dict(n_eff or {}), props=props, **pr)


# ------------------------------------------------------------------------------------------
# the scenes
# ------------------------------------------------------------------------------------------
TIE_DEPTHS = (2.0, 3.0, 5.0)

EXACT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)


def exact_size(N, W=203, H=117, n_absent=None):
    """I = V = N: one-tile Gaussians round-robin over the tiles, depths cycling over three values
    (ties everywhere), index order a seeded permutation of tile order, N // 3 (or n_absent) absent
    Gaussians interleaved.  Every owner has one record, every duplicate segment one slot."""
    b = Builder(W, H, seed=1000 + N, bg=(0.1, 0.2, 0.3))
    for k in range(N):
        b.add_tile(k % b.tiles, TIE_DEPTHS[(k // b.tiles) % 3], opacity=float(b.rng.uniform(0.05, 0.5)))
    n_absent = N // 3 if n_absent is None else n_absent
    return b.build(f"exact_{W}x{H}_{N}_{n_absent}", shuffle=True, n_absent=n_absent)


EXACT_TOTALS = (2047, 2048, 2049, 4096)


def exact_total(P):
    """P Gaussians in all, a quarter of them absent: the first depth-sort pass (which reads all P
    keys and drops the absent ones) has n = P exactly on / around the sort tile, while the later
    passes and the tile sort have n = V = I = P - P // 4."""
    return exact_size(P - P // 4, n_absent=P // 4)


def one_per_tile(W, H):
    """Every tile holds exactly one instance, all at z = 3: every instance is its own range."""
    b = Builder(W, H, seed=W * 1000 + H)
    for t in range(b.tiles):
        b.add_tile(t, 3.0, opacity=float(b.rng.uniform(0.2, 0.9)))
    return b.build(f"one_per_tile_{W}x{H}", shuffle=True, n_absent=b.tiles // 3)


def tie_clones(n_pairs=2600, W=203, H=117):
    """2 n_pairs Gaussians with ONE depth bit pattern over all tiles, as clone pairs: pair k is two
    Gaussians of identical mean, opacity 0.5 and different colours (what clone densification
    leaves behind).  Their order, hence the image, is decided by the index tie-break alone.  The
    second clone lies n_pairs indices after the first, so the tied keys span three sort tiles."""
    b = Builder(W, H, seed=77)
    cols = b.rng.random((2 * n_pairs, 3))
    for half in range(2):
        for k in range(n_pairs):
            b.add_tile(k % b.tiles, 3.0, opacity=0.5, colour=cols[half * n_pairs + k])
    name = f"tie_clones_{2 * n_pairs}" + ("" if (W, H) == (203, 117) else f"_{W}x{H}")
    return b.build(name, props=dict(n_pairs=n_pairs))


def reversed_scene(cs):
    """The same Gaussians in reverse index order (ties then resolve the other way)."""
    s = cs.scene
    flip = lambda t: torch.flip(t, [0]).contiguous()  # noqa: E731
    return gs_scenes.GaussianScene(flip(s.means3D), flip(s.opacities), flip(s.scales), flip(s.rotations), flip(s.shs),
                                   s.sh_degree)


DIGIT_BYTES = (0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF)


def digit_extremes(W=203, H=117):
    """Depth bit patterns whose three low bytes are each drawn from DIGIT_BYTES (radix digit bins
    0 and 255 and their neighbours, in every pass), top byte 0x3F / 0x40 / 0x41 (z in [0.5, 32)),
    every pattern twice (ties), in shuffled index order."""
    b = Builder(W, H, seed=5, bg=(0.3, 0.0, 0.1))
    k = 0
    for top in (0x3F, 0x40, 0x41):
        for b2 in DIGIT_BYTES:
            for b1 in DIGIT_BYTES:
                for b0 in DIGIT_BYTES:
                    bits = top << 24 | b2 << 16 | b1 << 8 | b0
                    for _ in range(2):
                        b.add_tile(k % b.tiles, depth_bits=bits, opacity=float(b.rng.uniform(0.05, 0.3)))
                        k += 1
    return b.build("digit_extremes", shuffle=True, n_absent=k // 3)


HOT_W, HOT_H, HOT_TILE = 80, 48, 7   # 5 x 3 tiles; tile 7 is the centre tile (its centre = the image's)
HOT_LENGTHS = (63, 64, 65, 127, 128, 129, 255, 256, 257)


def hot_tile(L, second=False):
    """One tile holding L faint entries (opacity 0.01), every other tile empty: one range over the
    whole list.  Each entry has alpha 0.00825 at the tile's four centre pixels, so after L <= 257
    of them T >= 0.99175^257 = 0.119 and no pixel stops early: n_eff = L.  second: a second hot
    tile of L entries, the last tile of the grid."""
    b = Builder(HOT_W, HOT_H, seed=L)
    hot = [HOT_TILE] + ([b.tiles - 1] if second else [])
    for t in hot:
        for k in range(L):
            b.add_tile(t, 2.0 + 0.01 * k)
    return b.build(f"hot_{L}{'_two' if second else ''}", shuffle=True, n_eff={t: L for t in hot}, props=dict(hot=hot))


STOP_N_EFF = (63, 64, 65, 128, 129)


def stop_edge(n_eff, variant="single"):
    """A tile whose compositing stops exactly n_eff entries into a list at least twice as long:
    k = n_eff - 2 faint entries, 4 covers, then a tail of n_eff + 70 faint entries behind.  At the
    pixels within 5 px of the centre a cover has alpha 0.99: the first leaves T <= 0.01, the second
    has T (1 - alpha) <= 1e-4 and stops the pixel (n_contrib = k + 1).  At the tile's corners
    (|d|^2 = 112.5) a cover has alpha 0.999 exp(-112.5 / 3200.6) = 0.9645: no faint entry reaches
    them (T = 1), the second cover leaves T = 1.26e-3 and is the last contributor, the third has
    T (1 - alpha) = 4.5e-5 and stops: n_contrib = k + 2 = n_eff, the tile's largest.
    Variants: "single" -- a one-tile image, so this tile holds cut_max and the tail;
    "tail_here" -- 5 x 3 tiles (the covers reach all of them), tail in the hot tile;
    "tail_elsewhere" -- the tail sits in the tile right of the hot one (behind the covers there)."""
    k = n_eff - 2
    if variant == "single":
        b = Builder(16, 16, seed=n_eff, bg=(0.2, 0.2, 0.2))
        hot = tail_tile = 0
    else:
        b = Builder(HOT_W, HOT_H, seed=n_eff, bg=(0.2, 0.2, 0.2))
        hot = HOT_TILE
        tail_tile = HOT_TILE + (variant == "tail_elsewhere")
    for j in range(k):
        b.add_tile(hot, 2.0 + 0.001 * j)
    for j in range(4):
        b.add_cover(hot, 4.0 + 0.1 * j)
    n_tail = n_eff + 70
    for j in range(n_tail):
        b.add_tile(tail_tile, 6.0 + 0.001 * j)
    return b.build(f"stop_{n_eff}_{variant}", shuffle=True, n_eff={hot: n_eff},
                   props=dict(hot=hot, tail_tile=tail_tile, n_tail=n_tail))


def big_owner(kind):
    """Full-screen Gaussians at 320 x 240: 300 instances (15 rows of 20) each.
    "straddle": 1898 one-tile Gaussians in front, so the owner's records are slots [1898, 2198):
        slot 2048 (the duplicate block / sort tile edge) falls in the middle of its row 7.
    "chunk_start": a full-screen Gaussian (rank 0, slots [0, 300)), 20 one-tile ones, then a second
        full-screen Gaussian of rank 21 whose records start at slot 320 = 5 * 64: exactly on a chunk
        base of its wave's sweep (which starts at slot 0), and it spans five chunks.
    "pair": two full-screen Gaussians at one depth, among one-tile Gaussians at that depth."""
    b = Builder(320, 240, seed={"straddle": 1, "chunk_start": 2, "pair": 3}[kind], bg=(0.0, 0.1, 0.0))
    rnd = lambda: float(b.rng.uniform(0.05, 0.2))  # noqa: E731
    big = []
    if kind == "straddle":
        for j in range(1898):
            b.add_tile(j % b.tiles, TIE_DEPTHS[j % 2], opacity=rnd())
        big.append(b.add_all_tiles(4.0, 0.3))
        for j in range(200):
            b.add_tile((7 * j) % b.tiles, 5.0, opacity=rnd())
    elif kind == "chunk_start":
        big.append(b.add_all_tiles(2.0, 0.3))
        for j in range(20):
            b.add_tile((13 * j) % b.tiles, 2.5, opacity=rnd())
        big.append(b.add_all_tiles(3.0, 0.3))
        for j in range(150):
            b.add_tile((7 * j) % b.tiles, 5.0, opacity=rnd())
    else:
        for j in range(100):
            b.add_tile((3 * j) % b.tiles, 3.0, opacity=rnd())
        big.append(b.add_all_tiles(3.0, 0.3))
        for j in range(100):
            b.add_tile((3 * j + 1) % b.tiles, 3.0, opacity=rnd())
        big.append(b.add_all_tiles(3.0, 0.4))
        for j in range(100):
            b.add_tile((3 * j + 2) % b.tiles, 3.0, opacity=rnd())
    cs = b.build(f"big_owner_{kind}", shuffle=True, n_absent=100, props=dict(big=big))
    cs.props["big"] = [int(cs.props["index_of"][h]) for h in big]
    return cs


# Grids past 1080p (8,160 tiles, 13 tile bits): the tile sort's digit plan follows the bit count of
# the tile count -- 14 bits 7 + 7, 15 bits 7 + 8, 16 bits 8 + 8, 17 bits 5 + 6 + 6 (the first
# three-pass tile sort: the sorted list ends in the other ping-pong buffer).  (W, H, tile bits).
LARGE_GRIDS = ((2059, 1013, 14), (2059, 2037, 15), (4107, 2037, 16), (4096, 4096, 16), (4107, 4085, 17))
GRID17 = (4107, 4085)   # 257 x 256 = 65,792 tiles, ragged last column and row
FEW_BIG_TILES = (0, 256, 65535, 65536, 65791)  # first tile, last of row 0, either side of 2^16, last


def tile_sort_plan(tiles):
    """Digit widths of the tile sort's passes, first pass first, restated from DESIGN.md: 8-bit
    digits at most, as few passes as the bit count of the tile ids allows, (nearly) equal widths
    with the narrower remainder first."""
    bits = max(1, (tiles - 1).bit_length())
    passes = -(-bits // 8)
    width = -(-bits // passes)
    first = bits - (passes - 1) * width
    return [first] + [width] * (passes - 1)


def few_big():
    """17 tile bits, few Gaussians with very many instances: three full-screen Gaussians (65,792
    instances each; depths 2, 3, 3: a tie) and five one-tile Gaussians at the tied depth in
    FEW_BIG_TILES, four absent ones.  P = 12, I = 197,381: more than a duplicate block's 2048
    slots per Gaussian on average, so the per-splat duplicate runs, and every owner's run is past
    65,535 records."""
    b = Builder(*GRID17, seed=17, bg=(0.05, 0.0, 0.1))
    big = [b.add_all_tiles(z, op) for z, op in ((2.0, 0.05), (3.0, 0.07), (3.0, 0.09))]
    for t in FEW_BIG_TILES:
        b.add_tile(t, 3.0, opacity=0.4)
    cs = b.build("few_big", shuffle=True, n_absent=4)
    cs.props["big"] = [int(cs.props["index_of"][h]) for h in big]
    return cs


def owner_among_many():
    """17 tile bits, balanced: one one-tile Gaussian per tile (depths cycling over three values) and
    one full-screen Gaussian at the middle depth, 1000 absent.  P = 66,793, I = 131,584: the
    look-back duplicate, where the one owner's 65,792 records cross 33 blocks of 2048 slots."""
    b = Builder(*GRID17, seed=18, bg=(0.0, 0.05, 0.05))
    for t in range(b.tiles):
        b.add_tile(t, TIE_DEPTHS[t % 3], opacity=float(b.rng.uniform(0.2, 0.9)))
    big = b.add_all_tiles(3.0, 0.05)
    cs = b.build("owner_among_many", shuffle=True, n_absent=1000)
    cs.props["big"] = [int(cs.props["index_of"][big])]
    return cs


def path_switch(P, W=203, H=117):
    """P Gaussians, all behind the camera except exactly 2049 one-tile Gaussians scattered through
    the index range (depths cycling over three values: ties).  Only the preprocess and the first
    depth-sort pass see P; P = LB_MAX_P is the last size of the look-back ordering path,
    LB_MAX_P + 1 the first of the large-scene path."""
    n = SORT_TILE + 1
    b = Builder(W, H, seed=P % 1000 + 9)
    for k in range(n):
        b.add_tile(k % b.tiles, TIE_DEPTHS[(k // b.tiles) % 3], opacity=float(b.rng.uniform(0.05, 0.5)))
    return b.build(f"path_switch_{P}", shuffle=True, n_absent=P - n, absent_kinds=("behind",))


def two_views(W=208, H=128):
    """One scene, two cameras whose exact counts differ: 2049 one-tile Gaussians for the identity
    camera A, all in tile columns >= 3 except one (z = 6, column 0).  Camera B is A moved right by
    16 * 6 / fx, which moves a Gaussian at depth z left by 6 / z whole tiles (z = 6, 3, 2: one, two,
    three tiles), so every Gaussian stays a one-tile Gaussian on a tile centre and exactly the one
    in column 0 leaves the image: I = V = 2049 in A, 2048 in B.  Returns (A's scene with its
    promises, camera B, B's promises)."""
    b = Builder(W, H, seed=31, bg=(0.1, 0.1, 0.1))
    depths = (6.0, 3.0, 2.0)
    cols = b.gx - 3
    for k in range(SORT_TILE):
        ty, tx = divmod(k % (cols * b.gy), cols)
        b.add_tile(ty * b.gx + 3 + tx, depths[k % 3], opacity=float(b.rng.uniform(0.05, 0.5)))
    lone = b.add_tile(2 * b.gx, 6.0, opacity=0.4)
    cs = b.build("two_views_A", shuffle=True, n_absent=600)
    cs.props["lone"] = int(cs.props["index_of"][lone])
    cam_b = gs_scenes.make_camera(np.eye(3), np.array([-TILE * 6.0 / b.fx, 0.0, 0.0]), W, H)
    z = bits_f32(cs.depth_bits).astype(np.float64)
    a_tile = np.full(cs.P, -1, np.int64)
    owners = cs.sorted_gid
    a_tile[cs.point_list] = np.repeat(np.arange(b.tiles), cs.list_len)
    shift = np.rint(6.0 / z).astype(np.int64)
    tx = a_tile % b.gx - shift
    b_tile = np.where((a_tile >= 0) & (tx >= 0), a_tile - shift, -1)
    assert len(owners) == SORT_TILE + 1
    pb = promises(cs.P, b.tiles, b_tile, np.zeros(cs.P, bool), cs.depth_bits)
    return cs, cam_b, pb


_FORWARD_CACHE: dict = {}


def oracle_scene(oracle, cam, sc, bg):
    return oracle.Scene(bg=bg, means3D=sc.means3D.numpy(), opacities=sc.opacities.numpy(), W=cam.image_width,
                        H=cam.image_height, viewmatrix=cam.world_view_transform.numpy(),
                        projmatrix=cam.full_proj_transform.numpy(), campos=cam.camera_center.numpy(),
                        tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2), shs=sc.shs.numpy(),
                        sh_degree=sc.sh_degree, scales=sc.scales.numpy(), rotations=sc.rotations.numpy())


CACHE_MAX_PIXELS = 1920 * 1080  # larger forwards (up to 200 MB an array) are computed per use


def oracle_forward(oracle, cs):
    """The oracle's forward with intermediates for a constructed scene, computed once per session
    and shared (read-only) by the CPU and GPU tests of that scene.  A forward above 1080p is not
    kept: whoever asks computes it and lets it go."""
    if cs.name in _FORWARD_CACHE:
        return _FORWARD_CACHE[cs.name]
    fw = oracle.forward(oracle_scene(oracle, cs.cam, cs.scene, cs.bg), intermediates=True)
    fw["bg"] = cs.bg
    for v in fw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    if cs.cam.image_width * cs.cam.image_height <= CACHE_MAX_PIXELS:
        _FORWARD_CACHE[cs.name] = fw
    return fw


_SCENE_CACHE: dict = {}


def cached(fn, *args):
    """Build a scene once per session (the builders are deterministic)."""
    key = (fn.__name__,) + args
    if key not in _SCENE_CACHE:
        _SCENE_CACHE[key] = fn(*args)
    return _SCENE_CACHE[key]


def all_scene_specs():
    """(id, function, args) of every constructed scene the GPU tests use."""
    specs = [(f"exact_{N}", exact_size, (N,)) for N in EXACT_SIZES]
    specs += [("exact_256x256_2048", exact_size, (2048, 256, 256))]
    specs += [(f"exact_total_{P}", exact_total, (P,)) for P in EXACT_TOTALS]
    specs += [(f"one_per_tile_{W}x{H}", one_per_tile, (W, H)) for W, H in ((203, 117), (256, 256), (272, 256))]
    specs += [("tie_clones", tie_clones, ()), ("digit_extremes", digit_extremes, ())]
    specs += [(f"hot_{L}", hot_tile, (L,)) for L in HOT_LENGTHS] + [("hot_257_two", hot_tile, (257, True))]
    specs += [(f"stop_{n}_single", stop_edge, (n, "single")) for n in STOP_N_EFF]
    specs += [("stop_65_tail_here", stop_edge, (65, "tail_here")),
              ("stop_129_tail_elsewhere", stop_edge, (129, "tail_elsewhere"))]
    specs += [(f"big_owner_{k}", big_owner, (k,)) for k in ("straddle", "chunk_start", "pair")]
    specs += [(f"path_switch_{P}", path_switch, (P,)) for P in (LB_MAX_P, LB_MAX_P + 1)]
    specs += [(f"one_per_tile_{W}x{H}", one_per_tile, (W, H)) for W, H, _ in LARGE_GRIDS]
    specs += [("tie_clones_80000_4107x4085", tie_clones, (40000,) + GRID17), ("few_big", few_big, ()),
              ("owner_among_many", owner_among_many, ())]
    return specs
