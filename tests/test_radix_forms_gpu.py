"""The radix sort in the forms a frame runs it (gswt_debug_sort_ex), at sizes of a few thousand items.

gswt_debug_sort drives launch_sort with the device count equal to the capacity, no payload, no key range and no range table.  A frame
never does: its count is below the capacity, GSWT_ORDER_DEPTH carries a second payload through k_radix_scatter<., 1> or <., 2>, the global
depth passes take their digits from key - kmin, and the last pass of the pair sort leaves every tile's [start, end) through atomicMax
and writes no keys.  Every expectation here is np.argsort(kind="stable") / np.searchsorted on the caller's arrays; all comparisons are
between integers.

Which forms a frame selects by itself: 512 threads at every capacity, payload form 1 up to 12 M pairs of capacity and form 2 above.  The
256-thread build, form 2 at small capacities and form 1 at large ones are reached through the hook's overrides only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 4096
KMIN = 0x3F7FFF37                  # non-zero low bytes just under 0x3F800000: key - kmin borrows across every byte
NS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8192, 3 * 4096 + 1, 40_000)
KEY_BITS = (5, 13, 16, 24, 32)
PAYLOADS = (0, 1, 2)               # none, k_radix_scatter<., 1>, k_radix_scatter<., 2>


def _caps(n):
    if n == 0:
        return [BLOCK]
    return sorted({n, n + 1, (n + BLOCK - 1) // BLOCK * BLOCK + BLOCK, 3 * n})


def _keys(rng, n_cap, lo, span):
    """n_cap keys in [lo, lo + span): runs of equal keys of skewed lengths, as pair keys come, between single random ones."""
    runs = rng.integers(0, span, size=n_cap // 3 + 1, dtype=np.uint64)
    k = np.repeat(runs, rng.integers(1, 6, size=runs.shape[0]))[:n_cap]
    if k.shape[0] < n_cap:
        k = np.concatenate([k, rng.integers(0, span, size=n_cap - k.shape[0], dtype=np.uint64)])
    return (k + np.uint64(lo)).astype(np.uint32)


def _payloads(rng, n_cap):
    # three different marks in the top bits, so a value, a payload word and an untouched tail word cannot be taken for one another
    vals = (np.arange(n_cap, dtype=np.uint32) | np.uint32(0x40000000))
    aux = rng.integers(0, 1 << 30, size=n_cap, dtype=np.uint64).astype(np.uint32) | np.uint32(0x80000000)
    return vals, aux


def _expect_ranges(sorted_keys, n_range_keys):
    ks = np.arange(n_range_keys)
    s = np.searchsorted(sorted_keys, ks, side="left")
    e = np.searchsorted(sorted_keys, ks, side="right")
    out = np.stack([s, e], axis=1)
    out[e == s] = 0                                        # an absent key reads (0, 0)
    return out.astype(np.uint32)


def _run(renderer, keys, vals, aux, n, key_bits, *, krange=None, n_range_keys=0, threads=0, aux_form=0, overflow=False, tag=""):
    """One sort through the hook, checked in full against numpy.  Returns nothing: asserts."""
    n_cap = keys.shape[0]
    k, v, x, rg = renderer.debug_sort_ex(keys, vals, aux if aux_form else None, n=n, overflow=overflow, key_bits=key_bits, krange=krange,
                                         n_range_keys=n_range_keys, threads=threads, aux_form=aux_form)
    seen = 0 if (overflow or n > n_cap) else n
    order = np.argsort(keys[:seen], kind="stable")
    assert np.array_equal(v[:seen], vals[:seen][order]), f"{tag}: vals"
    assert np.array_equal(v[seen:], vals[seen:]), f"{tag}: vals beyond n were written"
    if aux_form:
        assert np.array_equal(x[:seen], aux[:seen][order]), f"{tag}: the payload did not travel with its item"
        assert np.array_equal(x[seen:], aux[seen:]), f"{tag}: payload beyond n was written"
    if n_range_keys:
        assert k is None
        want = _expect_ranges(keys[:seen][order], n_range_keys)
        if not np.array_equal(rg, want):
            bad = int(np.nonzero((rg != want).any(axis=1))[0][0])
            raise AssertionError(f"{tag}: key {bad} has range {rg[bad].tolist()}, expected {want[bad].tolist()}")
    else:
        assert np.array_equal(k[:seen], keys[:seen][order]), f"{tag}: keys"
        assert np.array_equal(k[seen:], keys[seen:]), f"{tag}: keys beyond n were written"


@pytest.mark.parametrize("payload", PAYLOADS)
@pytest.mark.parametrize("threads", [512, 256])
def test_form_matrix(renderer, threads, payload):
    """threads x payload form (the parameters) x key range off / on x range table off / on x n x capacity x key bits.  The words of every
    buffer from n on -- including whole blocks past the last item -- come back as the caller's after any number of passes."""
    rng = np.random.default_rng(1000 * threads + payload)
    n_runs = 0
    for n in NS:
        for n_cap in _caps(n):
            vals, aux = _payloads(rng, n_cap)
            for key_bits in KEY_BITS:
                for with_range in (False, True):
                    for with_table in ((False, True) if key_bits <= 16 else (False,)):
                        span = 1 << key_bits
                        if with_range:
                            # (with the table the keys index it, so they stay small; without, they sit where depth keys sit)
                            lo = 1000 if with_table else (KMIN if key_bits < 32 else 0x00FFFF37)
                            span = min(span, (1 << 32) - lo)
                        else:
                            lo = 0
                        keys = _keys(rng, n_cap, lo, span)
                        _run(renderer, keys, vals, aux, n, key_bits, krange=(lo, lo + span - 1) if with_range else None,
                             n_range_keys=lo + span if with_table else 0, threads=threads, aux_form=payload,
                             tag=f"threads {threads} payload {payload} n {n} cap {n_cap} bits {key_bits} krange {with_range} table {with_table}")
                        n_runs += 1
    assert n_runs == (len(NS) - 1) * 4 * 16 + 16


def _constructed(key0, tail):
    """Sorted keys whose runs sit on chosen block boundaries (positions in brackets), n_range_keys = 200:
    a first run [0, 100) of key 0 or key 2; key 3 [100, 2100); key 5 [2100, 14388): starts inside block 0, covers blocks 1 and 2 whole,
    ends inside block 3; key 7 [14388, 16384): ends on block 3's last item; key 9 [16384, 20480): exactly block 4; key 11 [20480, 24575);
    key 12 the single last item of block 5 and key 13 the single first item of block 6; key 20 [24577, 25077); key 199 to the end --
    the end of block 6 (n = 7 blocks) or one item further (a last block of one item)."""
    runs = [(0 if key0 else 2, 100), (3, 2000), (5, 3 * BLOCK), (7, 4 * BLOCK - 14388), (9, BLOCK), (11, BLOCK - 1), (12, 1), (13, 1), (20, 500)]
    n = 7 * BLOCK + tail
    runs.append((199, n - sum(c for _, c in runs)))
    return np.concatenate([np.full(c, k, dtype=np.uint32) for k, c in runs])


@pytest.mark.parametrize("threads", [512, 256])
def test_ranges_on_constructed_runs(renderer, threads):
    rng = np.random.default_rng(77 + threads)
    for key0 in (True, False):
        for tail in (0, 1):
            sk = _constructed(key0, tail)
            n = sk.shape[0]
            assert (n % BLOCK == 0) == (tail == 0)
            want = _expect_ranges(sk, 200)
            assert want[5].tolist() == [2100, 14388] and want[7].tolist() == [14388, 16384] and want[9].tolist() == [16384, 20480]
            assert want[12].tolist() == [24575, 24576] and want[13].tolist() == [24576, 24577] and want[199, 1] == n
            assert (want[0, 1] > 0) == key0 and want[1].tolist() == [0, 0] and want[198].tolist() == [0, 0]
            for shuffled, key_bits in ((False, 8), (True, 8), (True, 13)):
                # sorted input on one pass: the blocks of the last pass are the blocks of the result, so the runs meet the block
                # boundaries exactly as drawn above; shuffled, every key's run is put together from many blocks
                keys = sk[rng.permutation(n)] if shuffled else sk
                for n_cap in (n, n + BLOCK + 1):
                    kk = np.concatenate([keys, rng.integers(0, 200, size=n_cap - n, dtype=np.uint64).astype(np.uint32)])
                    vals, aux = _payloads(rng, n_cap)
                    for payload in PAYLOADS:
                        _run(renderer, kk, vals, aux, n, key_bits, n_range_keys=200, threads=threads, aux_form=payload,
                             tag=f"key0 {key0} tail {tail} shuffled {shuffled} bits {key_bits} cap {n_cap} payload {payload}")


@pytest.mark.parametrize("threads", [512, 256])
def test_key_range_borrows_across_bytes(renderer, threads):
    """Digits of key - kmin with kmin = 0x3F7FFF37: spans of 2^k - 1, the range exactly the data's, wider than the data on both sides, and all
    keys equal.  The order is that of the raw keys."""
    rng = np.random.default_rng(99 + threads)
    n, n_cap = 3 * BLOCK + 1, 4 * BLOCK + 7
    vals, aux = _payloads(rng, n_cap)
    for k in (1, 8, 9, 16, 17, 24):
        key_bits = 8 * ((k + 7) // 8)
        span = (1 << k) - 1                                # kmax - kmin
        for form in ("exact", "wider", "equal"):
            if form == "exact":
                keys = _keys(rng, n_cap, KMIN, span + 1)
                keys[5], keys[n - 2] = KMIN, KMIN + span
            elif form == "wider":
                inner = max(1, span // 2)
                keys = _keys(rng, n_cap, KMIN + span // 4, inner)
                assert keys[:n].min() > KMIN or span < 4
                assert keys[:n].max() < KMIN + span
            else:
                keys = np.full(n_cap, KMIN + span // 2, dtype=np.uint32)
            for payload in PAYLOADS:
                _run(renderer, keys, vals, aux, n, key_bits, krange=(KMIN, KMIN + span), threads=threads, aux_form=payload,
                     tag=f"span 2^{k}-1 {form} payload {payload}")
    # the bytes really borrow: the digits of key - kmin are not the digits of key
    assert ((KMIN + 201) & 0xFF) < (KMIN & 0xFF) and (((KMIN + 201) - KMIN) >> 8) == 0 and ((KMIN + 201) >> 8) != (KMIN >> 8)
    assert (KMIN + 201) >> 16 != KMIN >> 16 and (KMIN + 201) >> 24 == KMIN >> 24


@pytest.mark.parametrize("threads", [512, 256])
def test_refused_counts_write_nothing(renderer, threads):
    """clamped_count: with the frame's overflow flag set, or a count above the capacity, the whole chain processes nothing -- every output
    word is the caller's and every range (0, 0).  (All buffers are allocated in full: nothing is out of bounds here.)  n = 0 likewise."""
    rng = np.random.default_rng(5 + threads)
    n_cap = 2 * BLOCK + 100
    vals, aux = _payloads(rng, n_cap)
    for key_bits, table in ((13, 0), (13, 1 << 13), (24, 0)):
        keys = _keys(rng, n_cap, 0, 1 << key_bits)
        for n, overflow in ((n_cap - 50, True), (n_cap, True), (n_cap + 1, False), (1 << 33, False), (3 * n_cap, True), (0, False), (0, True)):
            for payload in PAYLOADS:
                for krange in (None, (0, (1 << key_bits) - 1)):
                    _run(renderer, keys, vals, aux, n, key_bits, krange=krange, n_range_keys=table, threads=threads, aux_form=payload,
                         overflow=overflow, tag=f"n {n} overflow {overflow} bits {key_bits} table {table} payload {payload}")


@pytest.fixture(scope="module")
def large_input():
    """4.3 M items: more than 32 groups of 32 workgroups, so k_radix_supscan runs and k_radix_scatter takes the group prefixes from it.
    The reference order is computed once for both thread counts."""
    rng = np.random.default_rng(4300)
    n = 4_300_000
    n_cap = n + BLOCK + 1
    assert ((n_cap + BLOCK - 1) // BLOCK >> 5) + 1 > 32
    span = (1 << 21) + 12345                               # three passes of key - kmin, as the depths of a frame need
    keys = _keys(rng, n_cap, KMIN, span)
    vals, aux = _payloads(rng, n_cap)
    order = np.argsort(keys[:n], kind="stable")
    return dict(n=n, keys=keys, vals=vals, aux=aux, span=span, want_k=keys[:n][order], want_v=vals[:n][order], want_x=aux[:n][order])


@pytest.mark.parametrize("threads", [512, 256])
def test_group_prefix_path(renderer, large_input, threads):
    g = large_input
    n = g["n"]
    k, v, x, _ = renderer.debug_sort_ex(g["keys"], g["vals"], g["aux"], n=n, key_bits=24, krange=(KMIN, KMIN + g["span"] - 1),
                                        threads=threads, aux_form=1)
    assert np.array_equal(k[:n], g["want_k"]) and np.array_equal(v[:n], g["want_v"]) and np.array_equal(x[:n], g["want_x"])
    assert np.array_equal(k[n:], g["keys"][n:]) and np.array_equal(v[n:], g["vals"][n:]) and np.array_equal(x[n:], g["aux"][n:])


@pytest.mark.parametrize("n", [1, BLOCK, BLOCK + 1, 32 * BLOCK + 1])
def test_plain_hook_is_the_ex_hook(renderer, n):
    """gswt_debug_sort and gswt_debug_sort_ex (no payload, no key range, n = n_cap) run one helper: identical keys and values on the same
    random 32-bit keys, both numpy's stable order of the keys masked to key_bits (the bits above travel with their key).  Sizes: one item, a
    full block, a block and one item, and 33 workgroups -- two group rows of the workspace.  key_bits: one partial pass, two passes, four."""
    from gswt_renderer_amd import _lib as L
    lib = L.load()
    assert (32 * BLOCK + 1 + BLOCK - 1) // BLOCK == 33 and (33 >> 5) + 1 == 2
    rng = np.random.default_rng(2100 + n)
    keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    vals = np.arange(n, dtype=np.uint32) | np.uint32(0x40000000)
    for key_bits in (1, 9, 32):
        masked = keys & np.uint32((1 << key_bits) - 1)
        order = np.argsort(masked, kind="stable")
        k1, v1 = keys.copy(), vals.copy()
        assert lib.gswt_debug_sort(renderer._h, k1.ctypes.data, v1.ctypes.data, n, key_bits) == 0
        k2, v2, _, _ = renderer.debug_sort_ex(keys, vals, key_bits=key_bits)
        assert np.array_equal(k1, keys[order]) and np.array_equal(v1, vals[order]), f"gswt_debug_sort, n {n} bits {key_bits}"
        assert np.array_equal(k2, keys[order]) and np.array_equal(v2, vals[order]), f"gswt_debug_sort_ex, n {n} bits {key_bits}"
        assert np.array_equal(k1, k2) and np.array_equal(v1, v2)


def test_hook_refuses_inputs_it_cannot_run(renderer):
    """A key outside the range table or the key range, a range that needs more bits than the passes cover, an unknown workgroup width."""
    from gswt_renderer_amd.renderer import GSWTError
    keys = np.array([1, 2, 300, 4], dtype=np.uint32)
    vals = np.arange(4, dtype=np.uint32)
    for kw in (dict(key_bits=9, n_range_keys=256), dict(key_bits=9, krange=(0, 255)), dict(key_bits=8, krange=(0, 256)),
               dict(key_bits=9, threads=128), dict(key_bits=9, aux_form=1)):
        with pytest.raises(GSWTError):
            renderer.debug_sort_ex(keys, vals, **kw)
    # ... but a key the kernels never look at (beyond n) may be anything
    renderer.debug_sort_ex(keys, vals, n=2, key_bits=9, n_range_keys=256)
