"""The plain model of a residual image (bahip_frame_residual_image; DESIGN.md section 3, "Residual images"): the per-pair words of the
oracle (OracleBA.evaluate_pairs: associated, px, py, color_valid, depth_residual, depth_inv_stddev, desc_residual) grouped by pixel, the
keys formed as the definition forms them and their minimum taken -- no GPU.  The GPU tests (tests/test_gpu_residual_image.py) hold
the kernels to it bit for bit; tests/test_cpu_residual_image.py holds it to hand-made pair words and takes the census that makes the
GPU tests meaningful.  Also here: the compositing of shards and an equality of planes that treats every NaN as one word.  A plain
module: no fixtures, no conftest."""
import numpy as np

F = np.float32
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
EMPTY_INDEX = np.uint32(0xFFFFFFFF)
BEST, WORST = 0, 1
PLANES = ("key", "pairs", "index", "depth_residual", "inv_stddev", "desc_residual", "color_valid")
FLOAT_PLANES = ("depth_residual", "inv_stddev", "desc_residual")
ABS = np.uint32(0x7FFFFFFF)


def pair_words(associated, px, py, color_valid, depth_residual, depth_inv_stddev, desc_residual):
    """The seven per-pair words the model reads, one entry per surfel in buffer order (hand-made cases; from_oracle makes them of the
    oracle's).  Residuals are binary32 VALUES or uint32 bit patterns (any NaN payload goes through unchanged as bits)."""
    def f32(v, shape):
        v = np.asarray(v)
        return (v.astype(np.uint32).view(F) if v.dtype.kind == "u" else v.astype(F)).reshape(shape).copy()
    n = len(np.asarray(associated))
    return dict(associated=np.asarray(associated, bool).reshape(n), px=np.asarray(px, np.int64).reshape(n), py=np.asarray(py, np.int64).reshape(n),
                color_valid=np.asarray(color_valid, bool).reshape(n), depth_residual=f32(depth_residual, n),
                depth_inv_stddev=f32(depth_inv_stddev, n), desc_residual=f32(desc_residual, (n, 2)))


def from_oracle(ba, k, frame_T_global=None, indices=None):
    """The pair words of every surfel of the oracle `ba` (or of `indices`) against keyframe k's images, at the keyframe's own pose or
    at frame_T_global (12 floats)."""
    from oracle import binding as ob
    idx = np.arange(ba.surfels_size, dtype=np.uint32) if indices is None else np.asarray(indices, np.uint32)
    words = ba.evaluate_pairs(k, idx, frame_T_global)

    def field(name):
        offset, length = ob.OracleBA.PAIR_FIELDS[name]
        return words[:, offset:offset + length]
    as_float = lambda name: np.ascontiguousarray(field(name)).view(F)   # noqa: E731
    return dict(associated=field("associated")[:, 0] != 0, px=field("px")[:, 0].view(np.int32).astype(np.int64),
                py=field("py")[:, 0].view(np.int32).astype(np.int64), color_valid=field("color_valid")[:, 0] != 0,
                depth_residual=as_float("depth_residual")[:, 0].copy(), depth_inv_stddev=as_float("depth_inv_stddev")[:, 0].copy(),
                desc_residual=as_float("desc_residual").copy())


def keys_of(raw, index, select):
    """The definition's key of pairs with residual `raw` (binary32) and index plane value `index` (index_base + i)."""
    m = np.ascontiguousarray(raw, F).view(np.uint32) & ABS
    high = (ABS - m) if int(select) == WORST else m
    return (high.astype(np.uint64) << np.uint64(32)) | np.asarray(index, np.uint64)


def image(pairs, width, height, select=BEST, index_base=0):
    """The definition.  pairs: pair_words() / from_oracle(); returns a dict of the seven planes ((height, width); desc_residual
    (height, width, 2)) and `stats`: pairs (all associated), explained (pixels with a pair), multi (pixels with two or more), most
    (pairs in the fullest pixel), not_lowest (multi pixels whose winner is not their lowest index), ties (pixels where two pairs share
    the winning magnitude word), invalid_winners (winners without a valid colour pixel)."""
    w, h = int(width), int(height)
    sel = np.flatnonzero(pairs["associated"])
    px, py = pairs["px"][sel], pairs["py"][sel]
    assert np.all((px >= 0) & (px < w) & (py >= 0) & (py < h)), "an associated pair outside the image"
    pix = py * w + px
    index = sel.astype(np.uint64) + np.uint64(index_base)
    assert sel.size == 0 or int(index.max()) < 0xFFFFFFFF
    keys = keys_of(pairs["depth_residual"][sel], index, select)
    key = np.full(w * h, EMPTY_KEY, np.uint64)
    np.minimum.at(key, pix, keys)
    count = np.bincount(pix, minlength=w * h).astype(np.uint32)
    covered = key != EMPTY_KEY
    winner = np.where(covered, (key & np.uint64(0xFFFFFFFF)) - np.uint64(index_base), 0).astype(np.int64)
    zero = np.uint32(0)
    bits = lambda v: np.ascontiguousarray(v, F).view(np.uint32)   # noqa: E731
    if pairs["associated"].size:
        raw = np.where(covered, bits(pairs["depth_residual"])[winner], zero)
        inv = np.where(covered, bits(pairs["depth_inv_stddev"])[winner], zero)
        valid = covered & pairs["color_valid"][winner]
        desc = np.where(valid[:, None], bits(pairs["desc_residual"]).reshape(-1, 2)[winner], zero)
    else:
        raw = inv = np.zeros(w * h, np.uint32)
        valid = np.zeros(w * h, bool)
        desc = np.zeros((w * h, 2), np.uint32)
    lowest = np.full(w * h, EMPTY_KEY, np.uint64)
    np.minimum.at(lowest, pix, index)
    at_winning = (keys >> np.uint64(32)) == (key[pix] >> np.uint64(32))
    multi = count > 1
    stats = dict(pairs=int(sel.size), explained=int(covered.sum()), multi=int(multi.sum()), most=int(count.max()) if count.size else 0,
                 not_lowest=int(np.count_nonzero(multi & ((key & np.uint64(0xFFFFFFFF)) != lowest))),
                 ties=int(np.count_nonzero(np.bincount(pix[at_winning], minlength=w * h) > 1)),
                 invalid_winners=int(np.count_nonzero(covered & ~valid)))
    return dict(key=key.reshape(h, w), pairs=count.reshape(h, w),
                index=np.where(covered, key & np.uint64(0xFFFFFFFF), EMPTY_INDEX).astype(np.uint32).reshape(h, w),
                depth_residual=raw.astype(np.uint32).view(F).reshape(h, w), inv_stddev=inv.astype(np.uint32).view(F).reshape(h, w),
                desc_residual=np.ascontiguousarray(desc.astype(np.uint32)).view(F).reshape(h, w, 2),
                color_valid=valid.astype(np.uint8).reshape(h, w), stats=stats)


def magnitude_ties(pairs, width):
    """Pixels in which two associated pairs have the same |raw| word (whoever wins)."""
    sel = np.flatnonzero(pairs["associated"])
    pix = pairs["py"][sel] * int(width) + pairs["px"][sel]
    m = (np.ascontiguousarray(pairs["depth_residual"][sel], F).view(np.uint32) & ABS).astype(np.uint64)
    both = (pix.astype(np.uint64) << np.uint64(32)) | m
    return int(both.size - np.unique(both).size)


def composite(shards):
    """The planes of the union of several shards' planes (each made with its own index_base): the elementwise minimum of key, the sum of
    pairs, and per pixel the other planes of the shard whose key won."""
    keys = np.stack([s["key"] for s in shards])
    who = np.argmin(keys, axis=0)
    out = {"key": keys.min(axis=0), "pairs": np.sum([s["pairs"] for s in shards], axis=0).astype(np.uint32)}
    for name in PLANES[2:]:
        if all(name in s for s in shards):
            stack = np.stack([s[name] for s in shards])
            pick = who if stack.ndim == 3 else who[..., None]
            out[name] = np.take_along_axis(stack, np.broadcast_to(pick, stack.shape[1:])[None], axis=0)[0]
    return out


def words(plane, name=None):
    """A plane as unsigned words; in a binary32 plane every NaN becomes the one word 0x7fc00000 (+0.0 stays different from -0.0)."""
    a = np.ascontiguousarray(plane)
    if a.dtype != np.float32:
        return a
    w = a.view(np.uint32).copy()
    w[np.isnan(a)] = np.uint32(0x7FC00000)
    return w


def assert_same_bits(got, expected, what=""):
    """Every plane of `got` equals the expected one word for word (every NaN as one word), no pixel left out; names the first pixels
    that differ."""
    names = [n for n in PLANES if n in got]
    assert names and set(names) == {n for n in got if n != "stats"}, (what, sorted(got))
    for name in names:
        a, b = words(got[name]), words(expected[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
        bad = np.argwhere(a != b)
        assert bad.size == 0, (what, name, len(bad), [(tuple(int(v) for v in p), got[name][tuple(p)], expected[name][tuple(p)]) for p in bad[:5]])
