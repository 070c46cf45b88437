"""The dropout keep rule of csrc/common.h (mix32, philox4, dropout_keep, dropout_thresh, salted), restated on the host in numpy integer
arithmetic -- from the comments there, not from any kernel's output.  The instance tests take every mask from here:

    seed' = seed ^ salt                                  (salt: the per-step device word, 0 unless a step state was pulled)
    k     = mix32(lo32(seed') ^ (site * 0x9E3779B9)) ^ hi32(seed')
    a     = mix32((lo32(ctr) ^ k) + hi32(ctr) * 0x85EBCA6B),   b = mix32(a ^ 0xB5297A4D),   ctr = idx >> 2
    word  = (a << 16, a & 0xffff0000, b << 16, b & 0xffff0000)[idx & 3]       -- 16 random bits in the high half
    keep iff word >= thresh,  thresh = floor(p * 2^32) of the fp32 p the entry point receives (0: no dropout, everything is kept)

and a kept element is scaled by the fp32 quotient 1.0f / (1.0f - p).  The element index idx per kernel:
    LayerNorm forward, both backward sites, the bf16 copy     row * D + col
    casts, dropout_f32                                        the flat index
    softmax forward / backward                                row * ld + key      (ld, not Lk: a lane's 4 keys share one counter)"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    return np.asarray(x, dtype=np.uint64) & M32


def mix32(x):
    x = _u32(x)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def thresh(p):
    """dropout_thresh: the entry points take p as a C float"""
    p = float(np.float32(p))
    if p <= 0.0:
        return 0
    t = p * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def dscale(p):
    """what a kept element is multiplied by: 1.f / (1.f - p) in fp32 (1 without dropout)"""
    p = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - p)) if p > 0 else 1.0


def words(seed, site, idx, salt=0):
    """the 32-bit word of every element index (uint64 array holding values below 2^32)"""
    idx = np.asarray(idx, dtype=np.uint64)
    s = (int(seed) ^ int(salt)) & 0xFFFFFFFFFFFFFFFF
    k = int(mix32((s & 0xFFFFFFFF) ^ ((int(site) * 0x9E3779B9) & 0xFFFFFFFF))) ^ (s >> 32)
    ctr = idx >> np.uint64(2)
    a = mix32((((ctr & M32) ^ np.uint64(k)) + ((ctr >> np.uint64(32)) * np.uint64(0x85EBCA6B) & M32)) & M32)
    b = mix32(a ^ np.uint64(0xB5297A4D))
    w = idx & np.uint64(3)
    h = np.where(w < 2, a, b)
    return np.where((w & np.uint64(1)) == 0, (h << np.uint64(16)) & M32, h & np.uint64(0xFFFF0000))


def keep(seed, site, idx, p, salt=0):
    """bool array shaped as idx: the elements dropout site `site` keeps"""
    t = thresh(p)
    idx = np.asarray(idx, dtype=np.uint64)
    if t == 0:
        return np.ones(idx.shape, dtype=bool)
    return words(seed, site, idx, salt) >= np.uint64(t)


def flat_index(n):
    return np.arange(n, dtype=np.uint64)


def row_index(rows, cols, ld=None):
    """row * ld + col over a [rows, cols] tensor (LayerNorm: ld = D; softmax: cols = Lk or ld, ld = the row stride)"""
    ld = cols if ld is None else ld
    return np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(ld) + np.arange(cols, dtype=np.uint64)[None, :]


def keep_flat(seed, site, n, p, salt=0):
    return keep(seed, site, flat_index(n), p, salt)


def keep_rows(seed, site, rows, cols, p, ld=None, salt=0):
    return keep(seed, site, row_index(rows, cols, ld), p, salt)
