"""The images the send entries build from a block, restated in numpy from the layouts that kernels.h, encode.hip and SeqBuf / PackedBuf
(engine_internal.h) document in their comments -- not from the kernel bodies.  Every function returns the WHOLE span its builder
defines: guards, pads, repeated line ends and zero tails included (DESIGN.md 4.1').  tests/test_image_model.py shows that these
layouts are what the consumers address; tests/test_gpu_sequence_images.py compares every byte the device holds with them."""
import numpy as np

SEQ_PAD = 64          # guard bytes on both sides of a sequence buffer
SEQ_TAIL = 64         # ... and the room behind them for the k-mer window's 32-byte reads
PACK_PAD = 64         # pad bytes in front of / behind every 4-bit copy
PACK4_COPIES = 8      # 2 base phases x 4 byte shifts
PACK4_FRONT = 4       # bytes below 0 of every 4-bit copy that hold real bases
PACK2_PAYLOAD = 96    # new logical bytes per 128-byte line of a 2-bit phase copy
PACK2_BIAS = 96       # logical byte of the 4-base group 0
Q2_TAIL = 32          # zero bytes a window may read past the last base of a shifted 2-bit copy
GUARD, GUARD_ROWS, PAD4 = 0x47, 0x78, 0x77

A, C_, G, T, L, N, X, E = range(8)
_LUT = np.full(256, X, dtype=np.uint8)
for _ch, _c in (("A", A), ("C", C_), ("G", G), ("T", T), ("a", L), ("c", L), ("g", L), ("t", L), ("n", N), ("N", N), ("&", E)):
    _LUT[ord(_ch)] = _c


def codes(ascii_):
    return _LUT[np.asarray(ascii_, dtype=np.uint8)]


def rev_comp(c):
    r = np.asarray(c, dtype=np.uint8)[::-1]
    return np.where(r < 4, 3 - r, r).astype(np.uint8)


def _at(c, pos, outside):
    """c[pos] where pos lies inside the block, `outside` elsewhere (pos: int64 array of any shape)"""
    n = c.size
    inside = (pos >= 0) & (pos < n)
    out = np.full(pos.shape, outside, dtype=np.uint8)
    if n:
        out[inside] = c[pos[inside]]
    return out


def two_bit(c):
    """what a 2-bit copy stores for a code: codes >= 4 as 0"""
    return np.where(c < 4, c, 0).astype(np.uint8)


# ---- sequence buffers -----------------------------------------------------------------------------------------------
def seq_image(c, rows=False):
    """alloc[0, len + 2 * SEQ_PAD + 64): the codes (rows: code << 3) between guards; geometry (origin)"""
    c = np.asarray(c, dtype=np.uint8)
    out = np.full(c.size + 2 * SEQ_PAD + SEQ_TAIL, GUARD_ROWS if rows else GUARD, dtype=np.uint8)
    out[SEQ_PAD:SEQ_PAD + c.size] = (c << 3) if rows else c
    return out


# ---- the target's 2-bit phase copies in overlapped lines ------------------------------------------------------------------
def ref2_nphys(n):
    return ((n // 4 + 64 + PACK2_BIAS) // PACK2_PAYLOAD + 2) * 128


def ref2_logical(p):
    """logical byte of physical byte p: line p >> 7 holds the logical bytes [96 L, 96 L + 128)"""
    p = np.asarray(p, dtype=np.int64)
    return (p >> 7) * PACK2_PAYLOAD + (p & 127)


def ref2_image(c):
    """(4, nphys): physical byte p of copy k holds the bases 4 j + k .. 4 j + k + 3 of group j = logical(p) - 96, low bits first"""
    c2 = two_bit(np.asarray(c, dtype=np.uint8))
    nphys = ref2_nphys(c2.size)
    jj = ref2_logical(np.arange(nphys))
    nlog = int(jj.max()) + 1
    # the bases under the logical bytes of phase 0, 0 outside the block: logical byte jj starts at base 4 (jj - 96)
    under = np.zeros(4 * nlog + 8, dtype=np.uint8)
    assert 4 * PACK2_BIAS + c2.size <= 4 * nlog
    under[4 * PACK2_BIAS:4 * PACK2_BIAS + c2.size] = c2
    out = np.zeros((4, nphys), dtype=np.uint8)
    for k in range(4):
        logical = np.zeros(nlog, dtype=np.uint8)
        for b in range(4):
            logical |= under[k + b:k + b + 4 * nlog:4] << (2 * b)
        out[k] = logical[jj]
    return out


# ---- 4-bit copies -------------------------------------------------------------------------------------------------------
def pack4_nbytes(n):
    return n // 2 + 1


def pack4_stride(n):
    return (pack4_nbytes(n) + 2 * PACK_PAD + 127) & ~127


def pack4_image(c):
    """(8, stride), byte 0 of a copy at column PACK_PAD: in copy k + 2 s the bytes j in [-4, nbytes) hold code & 7 of base
    2 (j + s) + k in the low nibble and of the next base in the high nibble (7 outside the block); every other byte is 0x77"""
    c7 = np.asarray(c, dtype=np.uint8) & 7
    nb, stride = pack4_nbytes(c7.size), pack4_stride(c7.size)
    out = np.full((PACK4_COPIES, stride), PAD4, dtype=np.uint8)
    j = np.arange(-PACK4_FRONT, nb, dtype=np.int64)
    for s in range(4):
        for k in range(2):
            p0 = 2 * (j + s) + k
            out[k + 2 * s, PACK_PAD - PACK4_FRONT:PACK_PAD + nb] = _at(c7, p0, 7) | (_at(c7, p0 + 1, 7) << 4)
    return out


# ---- 2-bit shifted copies ---------------------------------------------------------------------------------------------
def q2_stride(n):
    return (n // 4 + 1 + Q2_TAIL + 127) & ~127


def q2_image(c, copies):
    """(copies, stride): dword w of copy p + 4 s holds the sixteen bases from (4 w + s) * 4 + p on, two bits each, low bits first;
    codes >= 4 and bases past the end are 0 (so a dword whose first base lies past the end is 0), and every byte is written"""
    c2 = two_bit(np.asarray(c, dtype=np.uint8))
    stride = q2_stride(c2.size)
    w = np.arange(stride // 4, dtype=np.int64)
    out = np.zeros((copies, stride // 4), dtype="<u4")
    for cp in range(copies):
        p, s = cp & 3, cp >> 2
        b0 = (4 * w + s) * 4 + p
        for k in range(16):
            out[cp] |= _at(c2, b0 + k, 0).astype("<u4") << np.uint32(2 * k)
    return out.view(np.uint8).reshape(copies, stride)


# ---- code presence and the class scores ---------------------------------------------------------------------------------
def presence(c):
    m = 0
    for v in np.unique(np.asarray(c, dtype=np.uint8) & 7):
        m |= 1 << int(v)
    return m


def class_scores(sub_mat, present_t, present_q):
    """The rule above class_scores() in options.hip: cls[x] bounds every matrix entry a base pair with (target code ^ query code) == x
    can have.  Codes >= 4 are stored as code 0 in the 2-bit copies, so a pair with such a code can show up in ANY class: its score joins
    every cls[x] -- but only for the codes that occur in the two blocks.  No score lies below -255."""
    m = np.asarray(sub_mat, dtype=np.int64).reshape(8, 8)
    cls = [max(int(m[r, r ^ x]) for r in range(4)) for x in range(4)]
    other = [int(m[r, q]) for r in range(8) for q in range(8)
             if (r >= 4 or q >= 4) and (r < 4 or (present_t >> r) & 1) and (q < 4 or (present_q >> q) & 1)]
    if other:
        cls = [max(v, max(other)) for v in cls]
    return [max(v, -255) for v in cls]


def expected(name, fwd_codes, copies=1):
    """the span of image `name` (engine.IMAGES) of a block with these forward codes, flat, and its geometry"""
    c = np.asarray(fwd_codes, dtype=np.uint8)
    if name.endswith("_rc"):
        c = rev_comp(c)
    kind = name[:-3] if name.endswith("_rc") else name
    if kind in ("ref", "query"):
        img = seq_image(c)
        geo = dict(bytes=img.size, stride=img.size, origin=SEQ_PAD, len=c.size, copies=1)
    elif kind == "ref8":
        img = seq_image(c, rows=True)
        geo = dict(bytes=img.size, stride=img.size, origin=SEQ_PAD, len=c.size, copies=1)
    elif kind in ("query4", "ref4"):
        img = pack4_image(c)
        geo = dict(bytes=img.size, stride=img.shape[1], origin=PACK_PAD, len=c.size, copies=PACK4_COPIES)
    elif kind == "ref2":
        img = ref2_image(c)
        geo = dict(bytes=img.size, stride=img.shape[1], origin=0, len=c.size, copies=4)
    elif kind in ("query2", "refq2"):
        img = q2_image(c, copies)
        geo = dict(bytes=img.size, stride=img.shape[1], origin=0, len=c.size, copies=copies)
    else:
        raise KeyError(name)
    return geo, img.reshape(-1)
