"""NumPy restatement of the dropout mask's definition (include/hicgat.h "feature dropout"), written
from the definition alone: every mask the dropout tests compare against comes from here, never
from the library.  uint64 arithmetic throughout."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays holding 32-bit words; key: two ints.  Returns the four output words."""
    c = [np.asarray(v, dtype=np.uint64) & _LO for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1),
             p0 & _LO]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def threshold(p):
    return min(int(math.floor(p * 4294967296.0)), 4294967295)


def scale(p):
    return np.float32(1.0 / (1.0 - p))


def keep_mask(rows, W, p, seed, step, site, row_offset=0):
    """bool [rows, W]: element (r, c) is kept iff word c % 4 of its quad's Philox call is >= T."""
    assert W % 4 == 0 and 0.0 <= p < 1.0
    W4 = W // 4
    R = np.uint64(row_offset) + np.arange(rows, dtype=np.uint64)[:, None]
    g = R * np.uint64(W4) + np.arange(W4, dtype=np.uint64)[None, :]
    words = philox4x32_10([g & _LO, g >> np.uint64(32), np.full_like(g, step & 0xFFFFFFFF), np.full_like(g, site)],
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    r = np.stack(words, axis=-1).reshape(rows, W)
    return r >= np.uint64(threshold(p))
