"""gswt_set_draws_merge_groups at the sizes and values where the merged-list build changes behaviour, entry for entry against
orc.sort_raw_depth_vec applied per group (which tests/test_sort_raw_depth_cpu.py pins to scene.rs:655-698):
  list entry = index in the member's raw-depth array + merge_offset[lod][tile], with the segment's lod in bits 28+,
  map id     = the member's map index.
Driven through the C ABI with synthetic raw-depth tables and groups: more than 256 groups built in one event (the segmented sort's
fourth radix pass), the 32 768-group cap, group lengths around the 1 024-entry block table, equal / negative / saturating depths,
and reuse of a previous event's lists (copied with their map ids rewritten) against GSWT_OPT_NO_MERGE_REUSE."""
import ctypes as C

import numpy as np
import pytest

from gswt_renderer_amd import _lib as L
from oracle import gswt_oracle as orc

pytestmark = pytest.mark.gpu

N_LOD, N_TILE, N_VIEW = 3, 16, 9
NLT = N_LOD * N_TILE
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


class Ctx:
    """A renderer with a one-splat scene (never rendered here) and a synthetic raw-depth table: raw[lt][view] (lt = lod * N_TILE + tile)."""

    def __init__(self, counts, gen, seed=0, upload_raw=True):
        from gswt_renderer_amd.renderer import GSWTRenderer
        self.r = GSWTRenderer(0)
        lists = [[[np.zeros(1, np.uint32)] * N_VIEW for _ in range(N_TILE)] for _ in range(N_LOD)]
        self.r.upload_scene(np.zeros((1, 8), np.uint32), lists, lists)
        rng = np.random.default_rng(seed)
        self.counts = np.ascontiguousarray(counts, dtype=np.uint32)
        assert self.counts.shape == (NLT,)
        self.offset = np.ascontiguousarray(rng.integers(0, 1 << 26, NLT), dtype=np.uint32)
        self.raw = [[np.ascontiguousarray(gen(lt, v, int(self.counts[lt]), rng), dtype=np.int32) for v in range(N_VIEW)] for lt in range(NLT)]
        ptrs = (C.c_void_p * (NLT * N_VIEW))(*[self.raw[lt][v].ctypes.data if self.counts[lt] else None for lt in range(NLT) for v in range(N_VIEW)])
        if upload_raw:
            self.r._check(self.r._lib.gswt_upload_raw_depth(self.r._h, ptrs, self.counts.ctypes.data, self.offset.ctypes.data))

    def close(self):
        self.r.close()

    def group_len(self, members):
        return sum(int(self.counts[l * N_TILE + t]) for _, lod, t, other in members for l in (lod, other) if l >= 0)

    def tables(self, groups, draws=True):
        """groups: [(view, [(map_index, lod, tile, other_lod), ...])] -> the C call's arrays and counts (D, nd, G, ng, M, nm)."""
        mem = [m for _, ms in groups for m in ms]
        G = (L.MergeGroup * max(1, len(groups)))()
        M = (L.MergeMember * max(1, len(mem)))()
        D = (L.Draw * max(1, len(groups)))()
        first = base = nd = 0
        for g, (view, ms) in enumerate(groups):
            G[g].view_id, G[g].first_member, G[g].n_members = view, first, len(ms)
            for k, (mi, lod, tile, other) in enumerate(ms):
                M[first + k].map_index, M[first + k].lod, M[first + k].tile, M[first + k].other_lod = mi, lod, tile, other
            n = self.group_len(ms)
            if draws and n:
                d = D[nd]
                d.tile.single_draw = 1
                d.tile.map_index = ms[0][0]
                d.merged, d.merged_group, d.merged_offset, d.merged_count = 1, g, base, n
                nd += 1
            first += len(ms)
            base += n
        return D, nd, G, len(groups), M, len(mem)

    def submit(self, groups, draws=True):
        """-> the C call's return code."""
        return self.r._lib.gswt_set_draws_merge_groups(self.r._h, *self.tables(groups, draws))

    def expect(self, groups):
        lists, maps = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
        for view, ms in groups:
            segs = [(self.raw[l * N_TILE + t][view], l * N_TILE + t, l, mi) for mi, lod, t, other in ms for l in (lod, other)
                    if l >= 0 and self.counts[l * N_TILE + t]]
            if not segs:
                continue
            seg, idx = orc.sort_raw_depth_vec([s[0] for s in segs])
            lt = np.array([s[1] for s in segs], np.int64)[seg]
            lod = np.array([s[2] for s in segs], np.uint32)[seg]
            lists.append((idx.astype(np.uint32) + self.offset[lt]) | (lod << np.uint32(28)))
            maps.append(np.array([s[3] for s in segs], np.uint32)[seg])
        return np.concatenate(lists), np.concatenate(maps)

    def check(self, groups, tag, draws=True):
        rc = self.submit(groups, draws)
        assert rc == L.GSWT_OK, (tag, rc, self.r._lib.gswt_last_error(self.r._h).decode())
        got_l, got_m = self.r.read_merged()
        want_l, want_m = self.expect(groups)
        assert got_l.shape == want_l.shape, (tag, got_l.shape, want_l.shape)
        bad = np.flatnonzero((got_l != want_l) | (got_m != want_m))
        assert bad.size == 0, f"{tag}: {bad.size} entries differ, first at {bad[:5].tolist()}: got {got_l[bad[:3]]} / {got_m[bad[:3]]}, want {want_l[bad[:3]]} / {want_m[bad[:3]]}"
        return got_l, got_m


def _uniform(lo=-200000, hi=200000):
    return lambda lt, v, n, rng: rng.integers(lo, hi, n, endpoint=True)


def _member(rng, mi):
    lod = int(rng.integers(0, N_LOD))
    other = int(rng.choice([-1, -1, lod + 1 if lod + 1 < N_LOD else -1, lod - 1]))
    return (mi, lod, int(rng.integers(0, N_TILE)), other)


def _random_groups(rng, n_groups, max_members=4):
    groups, mi = [], 0
    for _ in range(n_groups):
        k = int(rng.integers(1, max_members + 1))
        groups.append((int(rng.integers(0, N_VIEW)), [_member(rng, mi + j) for j in range(k)]))
        mi += k
    return groups


def _scene_counts():
    """Per-(lod, tile) counts of a synthetic tile set, as the default scene has them (lod0_count 600, / 4 per lod)."""
    from gswt_renderer_amd import synth
    verts = synth.make_tileset(n_lod=N_LOD, n_tile=N_TILE, lod0_count=600)
    return np.array([v.shape[0] for lod in verts for v in lod])


@pytest.mark.parametrize("n_groups", [255, 256, 257, 300, 4096])
def test_many_groups_in_one_event(n_groups):
    """Group ids take 8 bits up to 256 groups, 9 beyond: 16 + 9 key bits are a fourth 8-bit radix pass."""
    ctx = Ctx(_scene_counts(), _uniform())
    try:
        rng = np.random.default_rng(n_groups)
        ctx.check(_random_groups(rng, n_groups), f"{n_groups} groups")
        ctx.check(_random_groups(rng, n_groups), f"{n_groups} groups, no draws", draws=False)
    finally:
        ctx.close()


def test_32768_groups_and_the_cap():
    """Exactly 32 768 groups are built (15 group bits, 31 key bits); a 32 769th returns GSWT_ERR_CAPACITY and leaves the previous
    event's lists in place."""
    counts = np.random.default_rng(1).integers(1, 9, NLT)
    ctx = Ctx(counts, _uniform(-30, 30))
    try:
        rng = np.random.default_rng(2)
        groups = _random_groups(rng, 32768, max_members=2)
        want = ctx.check(groups, "32768 groups")
        assert ctx.r.merge_stats()[0] == 32768
        rc = ctx.submit(_random_groups(rng, 32769, max_members=1))
        assert rc == L.GSWT_ERR_CAPACITY
        got = ctx.r.read_merged()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        ctx.check(_random_groups(rng, 40), "after the refusal")
    finally:
        ctx.close()


def test_group_lengths_around_the_block_table():
    """Groups of 1, 1 023, 1 024, 1 025 and 4 097 entries, members whose raw-depth count is zero (no segment, between and around
    others), and an arena of several million entries with a group of about a million."""
    sizes = [1, 1023, 1024, 1025, 4097, 0, 0, 1, 2, 3, 255, 256, 257, 511, 512, 513]
    counts = np.zeros(NLT, np.int64)
    counts[:16] = sizes                                           # lod 0
    counts[16:32] = np.random.default_rng(3).integers(30000, 40000, 16)      # lod 1: the big arena (16 x 9 views x ~35k)
    counts[32:48] = [0, 1, 1024, 0] * 4
    ctx = Ctx(counts, _uniform(-10 ** 6, 10 ** 6))
    try:
        assert int(counts.sum()) * N_VIEW > 4_000_000
        g = []
        for t, n in enumerate(sizes):
            g.append((t % N_VIEW, [(t, 0, t, -1)]))                                   # one member of each length
        g.append((2, [(100, 0, 5, -1), (101, 0, 1, -1), (102, 0, 6, -1)]))            # zero, 1 023, zero
        g.append((3, [(103, 0, 5, -1), (104, 0, 6, -1)]))                             # nothing at all
        g.append((4, [(105, 0, 3, 1), (106, 0, 0, -1), (107, 2, 0, 1)]))              # Changing members: 1 025 + ~35k, 1, 0 + ~35k
        g.append((5, [(200 + t, 1, t, 2 if t % 2 else 0) for t in range(N_TILE)] * 2))  # ~1.1 M entries in one group
        g.append((6, [(300, 2, 2, 1), (301, 2, 14, -1)]))
        ctx.check(g, "lengths")
        assert ctx.group_len(g[-2][1]) > 1_000_000
    finally:
        ctx.close()


def test_equal_negative_and_saturating_depths():
    """All-equal depths (max == min: NaN buckets, read as 0), negative depths, and INT32_MIN / INT32_MAX, whose span wraps in i32."""
    kinds = {
        0: lambda n, rng: np.full(n, 7),
        1: lambda n, rng: np.full(n, -123456),
        2: lambda n, rng: rng.integers(-9000, -1, n),
        3: lambda n, rng: rng.choice([I32_MIN, I32_MAX, 0, -1, 1], n),
        4: lambda n, rng: rng.integers(2 ** 30, 2 ** 30 + 1000, n),
        5: lambda n, rng: rng.integers(-2 ** 30 - 1000, -2 ** 30, n),
        6: lambda n, rng: np.full(n, I32_MIN),
        7: lambda n, rng: np.full(n, I32_MAX),
        8: lambda n, rng: rng.integers(I32_MIN, I32_MAX, n, endpoint=True),
        9: lambda n, rng: rng.integers(-3, 3, n),
    }
    counts = [[1, 5, 700, 1500, 2000, 64, 33, 1, 3000, 2048, 9, 17, 1, 2, 3, 4][t] for lod in range(N_LOD) for t in range(N_TILE)]
    ctx = Ctx(counts, lambda lt, v, n, rng: kinds.get(lt % N_TILE, kinds[8])(n, rng))
    try:
        combos = [[0], [0, 16], [1], [1, 0], [2], [3], [3, 2], [4, 5], [5, 4, 9], [6], [7], [6, 7], [6, 0], [8], [8, 3], [9], [9, 1, 7],
                  [4, 7], [5, 6], [2, 9, 20]]
        groups = []
        for k, tiles in enumerate(combos):
            for v in (0, 4, 8):
                groups.append((v, [(10 * k + j, lt // N_TILE, lt % N_TILE, -1) for j, lt in enumerate(tiles)]))
        ctx.check(groups, "extreme depths")
        # the same groups with every member Changing to the next LOD down
        ch = [(v, [(mi, 0, t, 1) for mi, _, t, _ in ms]) for v, ms in groups]
        ctx.check(ch, "extreme depths, Changing")
    finally:
        ctx.close()


def _reuse_events(rng):
    """Two sort events: the second repeats a 257-member group, a 256-member group with every map id moved, a group whose map ids are
    permuted among its members, an unchanged group, and a few new ones."""
    big257 = [(i, int(rng.integers(0, N_LOD)), int(rng.integers(0, N_TILE)), -1) for i in range(257)]
    big256 = [(1000 + i, int(rng.integers(0, N_LOD)), int(rng.integers(0, N_TILE)), -1) for i in range(256)]
    perm = [_member(rng, 2000 + i) for i in range(7)]
    same = [_member(rng, 3000 + i) for i in range(3)]
    e1 = [(1, big257), (2, big256), (3, perm), (4, same)] + _random_groups(rng, 5)
    moved = [(mi + 5000, lod, t, o) for mi, lod, t, o in big256]
    ids = [m[0] for m in perm]
    permuted = [(ids[(k + 3) % len(ids)], lod, t, o) for k, (_, lod, t, o) in enumerate(perm)]
    e2 = _random_groups(rng, 3) + [(4, same), (1, big257), (3, permuted), (2, moved)]
    return e1, e2


def test_reuse_across_events_matches_no_reuse():
    """A 257-member group repeated in the next event is rebuilt, not copied; a 256-member group whose map ids all moved and a group
    whose map ids are permuted among its own members are copied with every map id rewritten.  Each event equals the oracle and
    the GSWT_OPT_NO_MERGE_REUSE result."""
    rng = np.random.default_rng(9)
    counts = np.random.default_rng(4).integers(0, 60, NLT)
    e1, e2 = _reuse_events(rng)
    results = {}
    for no_reuse in (0, 1):
        ctx = Ctx(counts, _uniform(), seed=5)
        try:
            ctx.r.set_option(L.GSWT_OPT_NO_MERGE_REUSE, no_reuse)
            ctx.check(e1, f"event 1 no_reuse={no_reuse}")
            b0, c0 = ctx.r.merge_stats()
            results[no_reuse] = ctx.check(e2, f"event 2 no_reuse={no_reuse}")
            b1, c1 = ctx.r.merge_stats()
            n_built = sum(1 for _, ms in e2 if ctx.group_len(ms))
            if no_reuse:
                assert (b1 - b0, c1 - c0) == (n_built, 0)
            else:
                # copied: the unchanged group, the moved 256-member group and the permuted one; the 257-member group is rebuilt
                n_copied = sum(1 for v, ms in e2[-4:] if len(ms) <= 256 and ctx.group_len(ms))
                assert n_copied == 3 and ctx.group_len(e2[-3][1]) and len(e2[-3][1]) == 257
                assert (b1 - b0, c1 - c0) == (n_built - n_copied, n_copied), (b1 - b0, c1 - c0, n_built)
        finally:
            ctx.close()
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])


def test_refused_events_leave_the_previous_lists_and_the_ctx_usable():
    """Every refusal of gswt_set_draws_merge_groups past the group cap -- a group's member range, view id, a member's lod or tile, a
    merged draw's count, group or single_draw flag (GSWT_ERR_BAD_ARG), and an event before gswt_upload_raw_depth (GSWT_ERR_STATE) --
    leaves the lists of the previous event current and byte-identical, and the events after them build and reuse as usual."""
    ctx = Ctx(_scene_counts(), _uniform())
    bare = Ctx(_scene_counts(), _uniform(), upload_raw=False)
    try:
        rng = np.random.default_rng(31)
        first = _random_groups(rng, 40)
        kept = [a.copy() for a in ctx.check(first, "first event")]

        def unchanged(tag):
            got = ctx.r.read_merged()
            assert np.array_equal(got[0], kept[0]) and np.array_equal(got[1], kept[1]), tag

        def group_past_members(D, nd, G, ng, M, nm): G[ng - 1].n_members += 1
        def view_out_of_range(D, nd, G, ng, M, nm): G[3].view_id = N_VIEW
        def lod_out_of_range(D, nd, G, ng, M, nm): M[5].lod = N_LOD
        def tile_out_of_range(D, nd, G, ng, M, nm): M[5].tile = N_TILE
        def count_off_by_one(D, nd, G, ng, M, nm): D[7].merged_count += 1
        def group_out_of_range(D, nd, G, ng, M, nm): D[7].merged_group = ng
        def no_single_draw(D, nd, G, ng, M, nm): D[7].tile.single_draw = 0

        for spoil in (group_past_members, view_out_of_range, lod_out_of_range, tile_out_of_range, count_off_by_one, group_out_of_range,
                      no_single_draw):
            t = ctx.tables(_random_groups(rng, 40))
            assert t[1] == 40 and t[3] == 40 and t[5] > 5        # (every count of the tile set is > 0: one merged draw per group)
            spoil(*t)
            rc = ctx.r._lib.gswt_set_draws_merge_groups(ctx.r._h, *t)
            assert rc == L.GSWT_ERR_BAD_ARG, (spoil.__name__, rc, ctx.r._lib.gswt_last_error(ctx.r._h).decode())
            unchanged(spoil.__name__)
        rc = bare.submit(_random_groups(rng, 40))
        assert rc == L.GSWT_ERR_STATE, (rc, bare.r._lib.gswt_last_error(bare.r._h).decode())
        assert bare.r.read_merged()[0].size == 0
        unchanged("an event refused on another context")

        ctx.check(_random_groups(rng, 40), "a fresh event after the refusals")
        reused0 = ctx.r.merge_stats()[1]
        ctx.check(first[:20] + _random_groups(rng, 20), "an event that repeats groups of the first one")
        assert ctx.r.merge_stats()[1] > reused0
    finally:
        ctx.close()
        bare.close()


def test_c5_map_event_with_hundreds_of_groups(renderer):
    """A real sort event on c5's 129x129 map with merge_topk 1 000 on a rough HeightMap (scattered merge candidates: a flat map's
    coalesce into fewer than 150 groups) builds more than 256 groups on the device: its lists equal the host's merged_gs_index /
    merged_map_id / merged_lod_id, as test_device_side_merged_lists_bit_exact checks at 9x9."""
    from gswt_renderer_amd import host, synth, workloads
    from gswt_renderer_amd.pipeline import GSWTPipeline
    w = workloads.WORKLOADS["c5"]
    cfg = dict(tile_map_half_wh=w["half"], **dict(w["user"], surface_type=host.SURFACE_HEIGHTMAP, height_map_wh=(64, 64),
                                                   height_map_scale=(1.0, 1.0, 4.0), merge_topk=1000, merge_dot_threshold=0.9))
    verts = synth.make_tileset(n_lod=3, n_tile=16, lod0_count=60)
    W, Hh = 480, 272
    pos, tgt = (3.0, -2.0, 14.0), (60.0, 90.0, 0.0)
    cu, vp = host.camera_uniforms(pos, tgt, (0, 0, 1), 45.0, 0.1, 2400.0, W, Hh)
    ph = GSWTPipeline(verts, host.user_data(**cfg), renderer=renderer)
    ph.update(pos, vp)
    s = ph.sort
    assert len(s.groups) > 256, len(s.groups)
    want_list, want_map, want_lod = s.merged_gs_index.copy(), s.merged_map_id.copy(), s.merged_lod_id.copy()
    has_lod = np.zeros(len(want_list), dtype=bool)
    for t in s.tiles:
        if t.merged and t.single_lod_id == -1:
            has_lod[t.merged_offset:t.merged_offset + t.merged_count] = True
    pd = GSWTPipeline(verts, host.user_data(**cfg), renderer=renderer, device_merge=True)
    pd.update(pos, vp)
    assert len(pd.sort.groups) == len(s.groups)
    got_packed, got_map = renderer.read_merged()
    assert got_packed.shape == want_list.shape
    assert np.array_equal(got_packed & ((1 << 28) - 1), want_list)
    assert np.array_equal(got_map, want_map)
    assert np.array_equal((got_packed >> 28)[has_lod], want_lod[has_lod])
    print(f"c5 map: {len(s.groups)} groups, {len(want_list)} merged entries")
