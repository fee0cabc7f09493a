"""A plain numpy model of the two tables every lookup stands on (DESIGN.md 4.2''):

  * the SEED POSITION TABLE (table.hip; common/seed_pos_table.cu:49-109): indexed positions by the rule of hazard H6, a window valid iff
    all `span` codes are below 4, the key taken in shape order with the first care position most significant, buckets ascending,
    inclusive index ends as copy_index_table returns them;
  * the NEIGHBOURHOOD TABLE (probe.hip): nbr_start = prefix sum of the merged run lengths, the run of key k = bucket(k) followed by
    bucket(k ^ (2 << 2t)) for the transition-enabled care positions t ascending (src/seeder.cpp:57-74's word order), and the 32-byte
    context record of every entry as kernels.h (CtxRec) and encode.hip state it: word 0 the seed start, bits 2k.. the code of base
    anchor + k (k < 54), bits 108 + 2k.. the complement of the code of base lend - 1 - k (k < 58); codes >= 4 and bases outside
    the block count as code 0.

Written from those statements, not from the kernels: no phase copies, no overlapped lines, no bit reversal."""
import numpy as np

CTX_R_BASES, CTX_L_BASES = 54, 58
CTX_DTYPE = np.dtype([("pos", "<u4"), ("w", "<u4", (7,))])

_CODE = np.full(256, 6, dtype=np.uint8)          # X
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
for _c in b"acgt":
    _CODE[_c] = 4                                # L (soft-masked)
_CODE[ord("N")] = _CODE[ord("n")] = 5
_CODE[ord("&")] = 7


def encode(ascii_u8):
    """common/parameters.h:4-13 on a uint8 array of ASCII."""
    return _CODE[np.asarray(ascii_u8, dtype=np.uint8)]


class Shape:
    def __init__(self, shape):
        self.text = shape
        self.span = len(shape)
        self.pos = np.array([i for i, ch in enumerate(shape) if ch in "1T"], dtype=np.int64)
        self.weight = int(self.pos.size)
        self.nkeys = 1 << (2 * self.weight)
        # bit t of the mask <=> the t-th care position is a 'T'; its word is key ^ (2 << 2t) (ntcoding.cpp:39-41, seeder.cpp:66)
        self.tmask = sum(1 << t for t, i in enumerate(self.pos) if shape[i] == "T")

    def masks(self, transition=True):
        """xor masks of the pieces of a run, in word order: the key itself, then one per transition-enabled care position"""
        return [0] + ([2 << (2 * t) for t in range(self.weight) if (self.tmask >> t) & 1] if transition else [])


def position_rule(length, span, step):
    """hazard H6 (seed_pos_table.cu:58-64) -> (start_offset, num_steps)"""
    step = max(int(step), 1)
    offset = (span + 1) % step
    return step - offset, ((length - span + offset) // step if length >= span else 0)


def seed_entries(codes, shape, step):
    """-> (keys, positions) of the valid indexed windows, ordered by (key, position): the table's content"""
    codes = np.asarray(codes, dtype=np.uint8)
    start, n = position_rule(codes.size, shape.span, step)
    p = start + max(int(step), 1) * np.arange(n, dtype=np.int64)
    bad = np.concatenate([[0], np.cumsum(codes >= 4)])
    p = p[(bad[p + shape.span] - bad[p]) == 0]
    key = np.zeros(p.size, dtype=np.int64)
    for j in range(shape.weight):
        key = (key << 2) | codes[p + shape.pos[j]]
    order = np.lexsort((p, key))
    return key[order], p[order].astype(np.uint32)


def index_ends(keys_sorted, nkeys):
    """inclusive bucket ends (the reference's d_index_table) of a sorted key list; uint32, nkeys words"""
    cnt = np.zeros(nkeys, dtype=np.uint32)
    if keys_sorted.size:
        u, c = np.unique(keys_sorted, return_counts=True)
        cnt[u] = c
    return np.cumsum(cnt, dtype=np.uint32)


def index_equal(index, keys_sorted):
    """index == index_ends(keys_sorted, index.size), without building a second table of 4^k words (a weight-14 one is 1 GiB): the
    ends are a step function that rises exactly at the non-empty keys, to the cumulative counts"""
    index = np.asarray(index)
    u, c = np.unique(np.asarray(keys_sorted, dtype=np.int64), return_counts=True)
    cum = np.cumsum(c)
    first = int(cum[0]) if u.size and u[0] == 0 else 0
    rises = np.flatnonzero(index[1:] != index[:-1]) + 1
    want = u[1:] if u.size and u[0] == 0 else u
    return int(index[0]) == first and np.array_equal(rises, want) and np.array_equal(index[u].astype(np.int64), cum)


def canonical(index, pos):
    """positions sorted inside every bucket of inclusive ends `index` (the reference's order inside a bucket is arrival order, H7)"""
    pos = np.asarray(pos)
    bucket = np.searchsorted(np.asarray(index), np.arange(pos.size, dtype=np.int64), side="right")
    return pos[np.lexsort((pos, bucket))]


# ---- neighbourhood table ---------------------------------------------------------------------------------------------------------------
def neighbourhood(keys_sorted, shape, transition=True):
    """The table of the sorted key list of a seed table (entry e of pos_table has key keys_sorted[e]).
    -> (nbr_start [4^k + 1] uint64, src: for every run entry in table order the pos_table entry it repeats)"""
    nkeys = shape.nkeys
    keys_sorted = np.asarray(keys_sorted, dtype=np.int64)
    u, c = np.unique(keys_sorted, return_counts=True)      # the non-empty buckets and their sizes
    first = np.concatenate([[0], np.cumsum(c)[:-1]]) if u.size else np.zeros(0, dtype=np.int64)
    masks = shape.masks(transition)
    run = np.zeros(nkeys, dtype=np.int64)
    for m in masks:
        run[u ^ m] += c                                     # (u ^ m are distinct keys: plain indexed add)
    nbr_start = np.concatenate([[0], np.cumsum(run)]).astype(np.uint64)
    src = np.zeros(int(nbr_start[-1]), dtype=np.int64)
    # entry e of bucket b (rank r) is entry pre_j(k) + r of the run of k = b ^ m_j, for every piece j; pre_j(k) = what the pieces
    # in front of j put into the run of k
    e = np.arange(keys_sorted.size, dtype=np.int64)
    rank = e - np.repeat(first, c)
    pre = np.zeros(nkeys, dtype=np.int64)
    base = nbr_start[:-1].astype(np.int64)
    for m in masks:
        kk = keys_sorted ^ m
        src[base[kk] + pre[kk] + rank] = e
        pre[u ^ m] += c
    return nbr_start, src


def context_records(codes, positions, seed_size, left_skip):
    """The CtxRec of an entry at every seed start in `positions` (kernels.h): lend = anchor - left_skip."""
    codes = np.asarray(codes, dtype=np.uint8)
    two = np.where(codes < 4, codes, 0).astype(np.uint8)
    pos = np.asarray(positions, dtype=np.int64)
    anchor = pos + seed_size
    lend = anchor - left_skip
    f = np.zeros((pos.size, CTX_R_BASES + CTX_L_BASES), dtype=np.uint8)
    r = anchor[:, None] + np.arange(CTX_R_BASES)[None, :]
    f[:, :CTX_R_BASES] = np.where(r < codes.size, two[np.minimum(r, codes.size - 1)], 0)
    le = lend[:, None] - 1 - np.arange(CTX_L_BASES)[None, :]
    f[:, CTX_R_BASES:] = 3 - np.where(le >= 0, two[np.maximum(le, 0)], 0)
    rec = np.zeros(pos.size, dtype=CTX_DTYPE)
    rec["pos"] = pos
    sh = (2 * np.arange(16, dtype=np.uint32))[None, :]
    for w in range(7):
        rec["w"][:, w] = np.bitwise_or.reduce(f[:, 16 * w:16 * w + 16].astype(np.uint32) << sh, axis=1)
    return rec


# ---- comparisons the CPU and the GPU tests share -----------------------------------------------------------------------------------------
SORT_MAX = 512  # table.hip: buckets above it keep their arrival order


def check_pos_table(pos, want_pos, want_keys, what=""):
    """buckets of up to SORT_MAX entries equal the model exactly, larger ones as sets"""
    pos, want_pos = np.asarray(pos), np.asarray(want_pos)
    assert pos.shape == want_pos.shape, (what, pos.shape, want_pos.shape)
    diff = np.flatnonzero(pos != want_pos)
    if diff.size == 0:
        return
    u, c = np.unique(want_keys, return_counts=True)
    size_of = dict(zip(u.tolist(), c.tolist()))
    bad_keys = np.unique(np.asarray(want_keys)[diff])
    for k in bad_keys.tolist():
        assert size_of[k] > SORT_MAX, (what, "bucket %d of %d entries is not the model's" % (k, size_of[k]))
        sel = np.asarray(want_keys) == k
        assert np.array_equal(np.sort(pos[sel]), want_pos[sel]), (what, "bucket %d holds other positions" % k)
