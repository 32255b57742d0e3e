"""The model of the tile mask table (kernels_tile_masks.hip; DESIGN.md section 3, "The tile mask table") for
tests/test_cpu_tile_masks.py, tests/test_gpu_tile_masks.py and tests/test_gpu_keyframe_sharded_observed_structure.py.  A plain module:
no fixtures, no conftest.

MODEL.  A is the K x N 0/1 matrix of tests/observed_covisibility.py (the oracle's per-pair `associated` flags).  T = ceil(N / 64)
tiles; an entry (t, k, m) exists iff m != 0, where bit i of m is A[k][64 t + i].  The table is (tile_first (T + 1,) uint32,
keyframes (E,) uint32, masks (E,) uint64), a tile's entries contiguous and ascending in k.  Under a keyframe partition of `world` ranks
keyframe k belongs to rank k % world; a rank's partial is the table of its own rows; the rank-major layout lists, per tile, the runs of
the ranks 0 .. world - 1 one after the other, each ascending; the canonical layout is the table itself.  The three reductions -- the
co-visibility matrix, the observer histogram, the observation lists -- are functions of the table alone.  All integers: every
comparison is an equality."""
import numpy as np

DEFAULT_ENTRY_SLICE = 1600000
DEFAULT_PAYLOAD_SLICE = 4000000


def tiles_of(n):
    return (int(n) + 63) // 64


def masks_of(A):
    """(K, T) uint64: bit i of [k][t] is A[k][64 t + i]."""
    A = np.asarray(A, bool)
    K, n = A.shape
    T = tiles_of(n)
    padded = np.zeros((K, T * 64), bool)
    padded[:, :n] = A
    bits = padded.reshape(K, T, 64).astype(np.uint64)
    return (bits << np.arange(64, dtype=np.uint64)[None, None, :]).sum(axis=2, dtype=np.uint64)


def table(A, rows=None):
    """The table of A, or of the rows `rows` of A alone (a rank's partial; the keyframe indices stay A's)."""
    A = np.asarray(A, bool)
    m = masks_of(A)
    K, T = m.shape
    keep = np.zeros(K, bool)
    keep[list(range(K)) if rows is None else list(rows)] = True
    first, ks, ms = [0], [], []
    for t in range(T):
        for k in range(K):
            if keep[k] and m[k, t]:
                ks.append(k)
                ms.append(m[k, t])
        first.append(len(ks))
    return np.array(first, np.uint32), np.array(ks, np.uint32), np.array(ms, np.uint64)


def owned(K, rank, world):
    return [k for k in range(K) if k % world == rank]


def partial(A, rank, world):
    """What rank `rank` of `world` lists: the table of its own keyframes."""
    return table(A, owned(np.asarray(A).shape[0], rank, world))


def listed(A, world):
    """Entries every rank lists."""
    return [len(partial(A, r, world)[1]) for r in range(world)]


def rank_major(A, world):
    """(tile_first, keyframes, masks): per tile the ranks' runs one after the other -- what the exchange of the entries leaves."""
    parts = [partial(A, r, world) for r in range(world)]
    T = tiles_of(np.asarray(A).shape[1])
    first, ks, ms = [0], [], []
    for t in range(T):
        for f, k, m in parts:
            ks.extend(k[f[t]:f[t + 1]].tolist())
            ms.extend(m[f[t]:f[t + 1]].tolist())
        first.append(len(ks))
    return np.array(first, np.uint32), np.array(ks, np.uint32), np.array(ms, np.uint64)


def tiles_to_reorder(A, world):
    """Tiles whose rank-major run is not ascending: where the merge has work."""
    first, ks, _ = rank_major(A, world)
    return sum(1 for t in range(len(first) - 1) if (np.diff(ks[first[t]:first[t + 1]].astype(np.int64)) < 0).any())


def interleaving_lists(A, world):
    """Surfels whose list, taken rank by rank, is not ascending: two of their keyframes k1 < k2 with rank(k1) > rank(k2)."""
    A = np.asarray(A, bool)
    count = 0
    for s in range(A.shape[1]):
        ks = np.flatnonzero(A[:, s])
        order = sorted(ks.tolist(), key=lambda k: (k % world, k))
        count += order != ks.tolist()
    return count


def dense(tab, K, n):
    """The inverse: A (K, n) from a table (asserts what makes it well formed)."""
    first, ks, ms = tab
    first = np.asarray(first).astype(np.int64)
    T = tiles_of(n)
    assert len(first) == T + 1 and first[0] == 0 and (np.diff(first) >= 0).all() and first[-1] == len(ks) == len(ms)
    A = np.zeros((K, T * 64), bool)
    for t in range(T):
        run = np.asarray(ks[first[t]:first[t + 1]]).astype(np.int64)
        assert (np.diff(run) > 0).all(), ("a tile that does not ascend", t)
        for k, m in zip(run, ms[first[t]:first[t + 1]]):
            assert int(m) != 0 and 0 <= k < K
            A[k, t * 64:(t + 1) * 64] = bits_of(m)
    assert not A[:, n:].any()
    return A[:, :n]


def bits_of(mask):
    """(64,) bool: bit i of a 64-bit ballot."""
    return ((np.uint64(int(mask)) >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def _popcount(x):
    return bin(int(x)).count("1")


def covisibility(tab, K):
    """The matrix from the table: per tile and pair of entries the popcount of the masks' intersection."""
    first, ks, ms = tab
    out = np.zeros((K, K), np.int64)
    for t in range(len(first) - 1):
        lo, hi = int(first[t]), int(first[t + 1])
        for a in range(lo, hi):
            for b in range(a, hi):
                v = _popcount(int(ms[a]) & int(ms[b]))
                out[ks[b], ks[a]] += v
                if a != b:
                    out[ks[a], ks[b]] += v
    return out


def covisibility_adds(tab, tiles=None):
    """Atomic adds of the reduction: pairs a <= b of a tile's entries whose masks meet, over `tiles` (default all)."""
    first, ks, ms = tab
    total = 0
    for t in (range(len(first) - 1) if tiles is None else tiles):
        lo, hi = int(first[t]), int(first[t + 1])
        total += sum(1 for a in range(lo, hi) for b in range(a, hi) if int(ms[a]) & int(ms[b]))
    return total


def lane_counts(tab, n):
    """Per surfel the entries of its tile that hold its bit: (n,) int64."""
    first, ks, ms = tab
    c = np.zeros(tiles_of(n) * 64, np.int64)
    for t in range(len(first) - 1):
        for m in ms[int(first[t]):int(first[t + 1])]:
            c[t * 64:(t + 1) * 64] += bits_of(m)
    return c[:n]


def histogram(tab, K, n, bins):
    """The observer histogram from the table."""
    first, ks, ms = tab
    c = lane_counts(tab, n)
    c = np.concatenate([c, np.zeros(tiles_of(n) * 64 - n, np.int64)])
    out = np.zeros((K, bins), np.int64)
    for t in range(len(first) - 1):
        b = np.minimum(c[t * 64:(t + 1) * 64] - 1, bins - 1)
        for e in range(int(first[t]), int(first[t + 1])):
            held = bits_of(ms[e])
            out[ks[e]] += np.bincount(b[held], minlength=bins)
    return out


def observations(tab, n):
    """(surfel_first (n + 1,) uint32, keyframes (P,) uint16) from the table."""
    first, ks, ms = tab
    c = lane_counts(tab, n)
    sf = np.concatenate([[0], np.cumsum(c)])
    out = np.zeros(int(sf[-1]), np.uint16)
    at = sf[:-1].copy()
    for t in range(len(first) - 1):
        for e in range(int(first[t]), int(first[t + 1])):
            for i in range(64):
                if (int(ms[e]) >> i) & 1:
                    out[at[t * 64 + i]] = ks[e]
                    at[t * 64 + i] += 1
    return sf.astype(np.uint32), out


def dealt_tiles(T, rank, world):
    return list(range(rank, T, world))


def _slices(words, slice_words):
    return -(-int(words) // int(slice_words)) if words else 0


def table_exchanges(E, entry_slice=DEFAULT_ENTRY_SLICE):
    """Exchanges that build the table under keyframe sharding: the counts, then the entries in slices (none when E = 0)."""
    return 1 + _slices(E, entry_slice)


def reduction_exchanges(E, entry_slice=DEFAULT_ENTRY_SLICE):
    """... of a matrix or a histogram call: the table, then the words."""
    return table_exchanges(E, entry_slice) + 1


def observation_exchanges(E, P, capacity, keyframes=True, depth=True, descriptor=True, entry_slice=DEFAULT_ENTRY_SLICE,
                          payload_slice=DEFAULT_PAYLOAD_SLICE):
    """... of a lists call: the table, then every payload plane asked for in slices of payload_slice 32-bit words (P words of depth_raw,
    2 P of descriptor_raw) -- when the planes are filled at all: keyframes given, 0 < P <= capacity."""
    total = table_exchanges(E, entry_slice)
    if keyframes and 0 < P <= capacity:
        total += (_slices(P, payload_slice) if depth else 0) + (_slices(2 * P, payload_slice) if descriptor else 0)
    return total
