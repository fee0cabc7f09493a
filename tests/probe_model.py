"""A plain numpy model of the front of a table-direct call (probe.hip / front.hip td_front; DESIGN.md 4.4'): what the position probe, the
compaction and the chunk plans must write for query positions [start, end) cut into chunks of `chunk` positions.

Written from the rules, not from the kernels:
  * the key of a query position is the key the seed table model gives that window (table_model.seed_entries at step 1; a window is
    valid iff all `span` codes are below 4), its run is the run of that key in table_model.neighbourhood;
  * the records are the non-empty positions in order: {exclusive sum of the run lengths, query position, run offset}, closed by the
    sentinel {hits, 0, 0}; head bit g is set iff a record starts at hit g; td_chunk[k] is the record whose hits hold hit 4096 k; the
    bounds triple of boundary c is the exclusive (hits, non-empty, valid) in front of position min(start + c chunk, end);
  * the plan of a chunk restates src/seed_filter.cu:718-745 over the inclusive prefix of hits per SEED WORD -- the words of every valid
    position in src/seeder.cpp:60-69 order with their plain bucket sizes, lower_bound - 1, limit_{i+1} = min(num_hits, prefix + MAX_HITS),
    the last iteration takes the rest -- and never looks at records or word boundaries "below a limit" as the kernel does;
  * a call is refused (return value 2^32 - 1) as td_front documents it: a chunk of more than TD_MAX_ITER iterations, a chunk with
    num_hits + MAX_HITS > 2^32 - 1 unless the call is the repeat masker's, more than MAX_SEGS iterations in the call, 2^32 - 1 hits or
    more, 2^32 - 1 seed words or more."""
import numpy as np

import table_model as M

TD_CHUNK_HITS = 4096
TD_MAX_ITER = 8
MAX_SEGS = 512
OVERFLOW = 0xFFFFFFFF
REFUSED = 0xFFFFFFFF
VALID = np.uint64(1 << 63)

PLAN_DTYPE = np.dtype([("hit_base", "<u8"), ("num_hits", "<u8"), ("upto", "<u8", (TD_MAX_ITER,)), ("num_valid", "<u4"), ("m_lo", "<u4"),
                       ("m_hi", "<u4"), ("n_iter", "<u4")])
BOUND_DTYPE = np.dtype([("hits", "<u8"), ("nonempty", "<u4"), ("valid", "<u4")])
REC_DTYPE = np.dtype([("prefix", "<u4"), ("qpos", "<u4"), ("off", "<u8")])


def position_keys(codes, shape):
    """key of the window at every position 0 .. len - span of `codes` (-1: not a valid window; positions whose window leaves the
    sequence are not listed).  seed_entries skips position 0 by the table's rule (hazard H6): one base in front moves it to 1."""
    codes = np.asarray(codes, dtype=np.uint8)
    n = max(codes.size - shape.span + 1, 0)
    keys = np.full(n, -1, dtype=np.int64)
    k, p = M.seed_entries(np.concatenate([np.zeros(1, dtype=np.uint8), codes]), shape, 1)
    keys[p.astype(np.int64) - 1] = k
    return keys


class Table:
    """what a call needs of the target: plain bucket sizes and the runs of the neighbourhood table"""

    def __init__(self, target_codes, shape, step, transition=True):
        self.shape, self.transition = shape, bool(transition)
        keys, _ = M.seed_entries(target_codes, shape, step)
        self.masks = np.array(shape.masks(transition), dtype=np.int64)
        self.bucket = np.bincount(keys, minlength=shape.nkeys).astype(np.int64)
        self.nbr_start, _ = M.neighbourhood(keys, shape, transition)
        self.run = np.diff(self.nbr_start.astype(np.int64))
        self.words = int(self.masks.size)


def plan_from_words(prefix, max_hits, rm):
    """src/seed_filter.cu:718-745 on the inclusive prefix of hits per seed word -> (n_iter or OVERFLOW, the hit offsets at which the
    iterations end).  max_hits is the int the reference compares and adds as unsigned."""
    num_seeds = int(prefix.size)
    num_hits = int(prefix[-1]) if num_seeds else 0                                      # :716
    if num_hits == 0:
        return 0, []
    maxh = int(max_hits) & 0xFFFFFFFF
    if num_hits < maxh:                                                                 # :721-724
        num_iter, limit = 2, num_hits
    else:                                                                               # :725-728
        num_iter, limit = num_hits // maxh + 2, maxh
    if num_iter > TD_MAX_ITER or (not rm and num_hits + maxh > 0xFFFFFFFF):
        return OVERFLOW, []
    limit_pos = []
    for _ in range(num_iter - 1):                                                       # :732-739
        pos = int(np.searchsorted(prefix, limit, side="left")) - 1                      # lower_bound - 1; -1: hazard H5, read as "no hits"
        limit_pos.append(pos)
        limit = min((int(prefix[pos]) if pos >= 0 else 0) + maxh, num_hits)
    limit_pos.append(num_seeds - 1)                                                     # :741
    if limit_pos[-1] == limit_pos[-2]:                                                  # :743
        limit_pos.pop()
    return len(limit_pos), [int(prefix[p]) if p >= 0 else 0 for p in limit_pos]


def word_prefix(table, keys):
    """inclusive prefix of hits per seed word of the valid positions with these keys, words in emission order"""
    keys = np.asarray(keys, dtype=np.int64)
    sizes = table.bucket[keys[:, None] ^ table.masks[None, :]]
    return np.cumsum(sizes.reshape(-1))


def probe(table, qkeys, start, end, chunk, num_chunks, max_hits, rm=False, head_bits=True):
    """-> dict of everything the front writes for positions [start, end) (already clipped) in `num_chunks` chunks"""
    n = end - start
    key = qkeys[start:end]
    valid = key >= 0
    cnt = np.zeros(n, dtype=np.int64)
    off = np.zeros(n, dtype=np.uint64)
    cnt[valid] = table.run[key[valid]]
    off[valid] = table.nbr_start[key[valid]]
    ex_hits = np.concatenate([[0], np.cumsum(cnt)])
    ex_ne = np.concatenate([[0], np.cumsum(cnt > 0)])
    ex_valid = np.concatenate([[0], np.cumsum(valid)])
    hits, ne = int(ex_hits[-1]), int(ex_ne[-1])
    out = {"hits": hits, "num_records": ne, "words": table.words, "num_chunks": num_chunks,
           "t_off": np.where(valid, off | VALID, np.uint64(0)), "t_cnt": cnt.astype(np.uint32)}
    idx = np.flatnonzero(cnt > 0)
    rec = np.zeros(ne + 1, dtype=REC_DTYPE)
    rec["prefix"][:ne] = ex_hits[idx] & 0xFFFFFFFF
    rec["qpos"][:ne] = start + idx
    rec["off"][:ne] = off[idx]
    rec["prefix"][ne] = hits & 0xFFFFFFFF
    out["records"] = rec
    if head_bits:
        bits = np.zeros(((hits + 63) >> 6) * 2 + 16, dtype=np.uint32)
        g = ex_hits[idx]
        np.bitwise_or.at(bits, g >> 5, (np.uint32(1) << (g & 31).astype(np.uint32)))
        out["head_bits"] = bits
    else:
        out["head_bits"] = np.zeros(0, dtype=np.uint32)
    # the record whose hit range [prefix, prefix + count) holds hit 4096 k
    marks = np.arange((hits + TD_CHUNK_HITS - 1) // TD_CHUNK_HITS, dtype=np.int64) * TD_CHUNK_HITS
    out["td_chunk"] = (np.searchsorted(ex_hits[idx], marks, side="right") - 1).astype(np.uint32)
    b = np.minimum(start + np.arange(num_chunks + 1, dtype=np.int64) * chunk, end) - start
    bounds = np.zeros(num_chunks + 1, dtype=BOUND_DTYPE)
    bounds["hits"], bounds["nonempty"], bounds["valid"] = ex_hits[b], ex_ne[b], ex_valid[b]
    out["bounds"] = bounds
    plans = np.zeros(num_chunks, dtype=PLAN_DTYPE)
    seg_end, refused, total_iter = [], False, 0
    for c in range(num_chunks):
        lo, hi = int(b[c]), int(b[c + 1])
        p = plans[c]
        p["hit_base"], p["num_hits"] = ex_hits[lo], ex_hits[hi] - ex_hits[lo]
        p["num_valid"], p["m_lo"], p["m_hi"] = ex_valid[hi] - ex_valid[lo], ex_ne[lo], ex_ne[hi]
        n_iter, ends = plan_from_words(word_prefix(table, key[lo:hi][valid[lo:hi]]), max_hits, rm)
        p["n_iter"] = n_iter
        p["upto"][:] = ex_hits[lo]
        if n_iter == OVERFLOW:
            refused = True
            continue
        if not rm and int(p["num_hits"]) > 0xFFFFFFFF:
            refused = True
        p["upto"][:n_iter] = int(ex_hits[lo]) + np.array(ends, dtype=np.int64)
        seg_end += [int(ex_hits[lo]) + e for e in ends]
        total_iter += n_iter
    out["plans"] = plans
    out["num_seg_end"] = total_iter
    out["seg_end"] = np.array(seg_end[:MAX_SEGS], dtype=np.uint64)
    nvalid = int(ex_valid[-1])
    if total_iter > MAX_SEGS or hits >= 0xFFFFFFFF or nvalid * table.words >= 0xFFFFFFFF:
        refused = True
    out["ret"] = REFUSED if refused else nvalid * table.words
    return out


ARRAYS = ("t_off", "t_cnt", "records", "head_bits", "td_chunk", "bounds", "plans", "seg_end")
SCALARS = ("ret", "words", "hits", "num_records", "num_chunks", "num_seg_end")


def differences(got, want):
    """names of the fields of a sa_probe_call result that are not exactly the model's (with where they first differ)"""
    bad = []
    for k in SCALARS:
        if int(got[k]) != int(want[k]):
            bad.append("%s: %d != %d" % (k, got[k], want[k]))
    for k in ARRAYS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape:
            bad.append("%s: %s entries != %s" % (k, a.shape, b.shape))
        elif a.dtype.names:
            for f in a.dtype.names:
                d = np.flatnonzero((a[f] != b[f]).reshape(a.shape[0], -1).any(axis=1))
                if d.size:
                    bad.append("%s.%s: %d differ, first at %d: %s != %s" % (k, f, d.size, d[0], a[f][d[0]], b[f][d[0]]))
        else:
            d = np.flatnonzero(a != b)
            if d.size:
                bad.append("%s: %d differ, first at %d: %s != %s" % (k, d.size, d[0], a[d[0]], b[d[0]]))
    return bad
