"""Expected per-tile pair lists of a frame, from the CPU oracle alone (no tests here).

The oracle blends back to front: in GSWT_ORDER_REFERENCE in entry order (draw after draw, each draw's list in order), in
GSWT_ORDER_DEPTH in orc_render's stable sort by descending depth, equal depths in entry order.  The HIP path composites front to back,
so the list of a screen tile is the oracle's blend sequence REVERSED and restricted to the entries whose rectangle of 16x16 pixel
blocks (oracle.pair_rects) holds the tile.  Everything here is integers: entry indices, tile numbers, positions.

Entries are numbered in draw order over the ORACLE's draws.  The product numbers its own list entries the same way, but a static draw
whose valid_lod_id is its base list's LOD reads the LOD-filtered copy of that list (the entries another LOD id makes invisible
anyway are not in it) unless GSWT_OPT_NO_LOD_PREFILTER is set: product_entry_map translates."""
from __future__ import annotations

import numpy as np

ORDER_REFERENCE, ORDER_DEPTH = 0, 1


class PairLists:
    """Per tile t the slice pairs[start[t]:end[t]] of one list of entry indices, front to back."""

    def __init__(self, start, end, pairs):
        self.start = np.asarray(start, dtype=np.int64)
        self.end = np.asarray(end, dtype=np.int64)
        self.pairs = np.asarray(pairs, dtype=np.int64)

    @classmethod
    def from_lists(cls, lists):
        lens = np.array([len(l) for l in lists], dtype=np.int64)
        end = np.cumsum(lens)
        pairs = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]) if len(lists) else np.zeros(0, np.int64)
        return cls(end - lens, end, pairs)

    @classmethod
    def from_gpu(cls, ranges, pairs):
        """read_ranges() ([n_tiles, 2] (start, end), (0, 0) for a tile without pairs) + read_pairs()."""
        r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
        return cls(r[:, 0], r[:, 1], pairs)

    @property
    def n_tiles(self):
        return self.start.shape[0]

    def lengths(self):
        return self.end - self.start

    def total(self):
        return int(self.lengths().sum())

    def tile(self, t):
        return self.pairs[self.start[t]:self.end[t]]

    def lists(self):
        return [self.tile(t).copy() for t in range(self.n_tiles)]


def blend_sequence(rects, order_mode):
    """Entry indices in the order the oracle blends them (back to front)."""
    idx = np.nonzero(rects["visible"] != 0)[0]
    if order_mode == ORDER_DEPTH:
        # descending depth, equal depths in entry order (orc_render's merge takes the right run only on `>`); a visible depth is in [0, 1]
        d = rects["depth"][idx].astype(np.float64)
        idx = idx[np.argsort(-d, kind="stable")]
    return idx


def expected_lists(rects, order_mode, tiles_x, tiles_y) -> PairLists:
    """oracle.pair_rects(...) -> the frame's lists over the tiles_x x tiles_y screen tiles (tile = ty * tiles_x + tx)."""
    seq = blend_sequence(rects, order_mode)[::-1]                  # front to back
    r = rects[seq]
    w = np.maximum(r["tx1"].astype(np.int64) - r["tx0"] + 1, 0)
    h = np.maximum(r["ty1"].astype(np.int64) - r["ty0"] + 1, 0)
    cnt = w * h
    assert not cnt.size or (r["tx1"][cnt > 0].max() < tiles_x and r["ty1"][cnt > 0].max() < tiles_y)
    rep = np.repeat(np.arange(seq.shape[0]), cnt)                   # one row per (entry, tile), entries in composite order
    off = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    tx = r["tx0"][rep] + off % np.maximum(w[rep], 1)
    ty = r["ty0"][rep] + off // np.maximum(w[rep], 1)
    tile = ty.astype(np.int64) * tiles_x + tx
    o = np.argsort(tile, kind="stable")
    ts = tile[o]
    n_tiles = tiles_x * tiles_y
    start = np.searchsorted(ts, np.arange(n_tiles), side="left")
    end = np.searchsorted(ts, np.arange(n_tiles), side="right")
    return PairLists(start, end, seq[rep][o])


def shard_tiles(tiles_x, tiles_y, shard=None, band_px=0):
    """Global tile number of every shard-local tile, in local order.  shard: None (the whole frame), (index, count) = interleaved tile
    rows -- row ty belongs to shard ty % count and is row ty // count there --, or (index, count, "cols") = a band of tile columns,
    band_px = gswt_shard_cols_padded(width, count) pixels wide: columns [index * band_px / 16, (index + 1) * band_px / 16)."""
    if shard is None:
        return np.arange(tiles_x * tiles_y)
    index, count = int(shard[0]), int(shard[1])
    if len(shard) > 2 and shard[2] in ("cols", "columns"):
        assert band_px > 0 and band_px % 16 == 0
        bt = band_px // 16
        cols = np.arange(min(index * bt, tiles_x), min((index + 1) * bt, tiles_x))
        rows = np.arange(tiles_y)
    else:
        cols = np.arange(tiles_x)
        rows = np.arange(index, tiles_y, count)
    return (rows[:, None] * tiles_x + cols[None, :]).reshape(-1)


def shard_lists(full: PairLists, tiles_x, tiles_y, shard=None, band_px=0) -> PairLists:
    """The frame's lists -> the lists of one shard, in its local tile order."""
    return PairLists.from_lists([full.tile(t) for t in shard_tiles(tiles_x, tiles_y, shard, band_px)])


def product_entry_map(product_draws, orc_draws, prefilter=True):
    """Oracle entry index of every product list entry (see the module text)."""
    out, base = [], 0
    for g, d in zip(product_draws, orc_draws):
        n = int(np.asarray(d.gs_index).shape[0])
        idx = base + np.arange(n, dtype=np.int64)
        if prefilter and not g.merged and g.tile.valid_lod_id >= 0 and int(g.tile.valid_lod_id) == int(g.base_lod):
            idx = idx[np.asarray(d.lod_id) == g.tile.valid_lod_id]
        out.append(idx)
        base += n
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def compare(want: PairLists, got: PairLists):
    """None when every tile's list is the same, else a sentence naming the first differing tile and position."""
    if want.n_tiles != got.n_tiles:
        return f"{got.n_tiles} tiles, expected {want.n_tiles}"
    n = got.pairs.shape[0]
    bad = np.nonzero((got.start < 0) | (got.end < got.start) | (got.end > n))[0]
    if bad.size:
        t = int(bad[0])
        return f"tile {t}: range ({int(got.start[t])}, {int(got.end[t])}) is not a slice of a list of {n} pairs"
    for t in range(want.n_tiles):
        a, b = want.tile(t), got.tile(t)
        if a.shape[0] == b.shape[0] and np.array_equal(a, b):
            continue
        m = min(a.shape[0], b.shape[0])
        d = np.nonzero(a[:m] != b[:m])[0]
        if d.size:
            p = int(d[0])
            return f"tile {t}, position {p}: entry {int(b[p])}, expected {int(a[p])} (list lengths {b.shape[0]} / {a.shape[0]})"
        return f"tile {t}, position {m}: list of {b.shape[0]} pairs, expected {a.shape[0]}"
    if got.total() != n:
        return f"the tiles' slices hold {got.total()} pairs, the list {n}"
    return None
