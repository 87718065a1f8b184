"""NumPy restatement of the attention-dropout mask (include/hicgat.h "attention dropout"), written from
the definition alone (TEST INFRASTRUCTURE ONLY): one Philox4x32-10 call per edge with counter
(destination row i, source row j, step, site | 2^31), keyed by the seed; head hh uses output word hh;
kept iff the word >= T.  Every mask the attention-dropout tests compare against comes from here, never
from the library."""
import numpy as np

from philox_ref import philox4x32_10, scale, threshold  # noqa: F401  (scale: re-exported for the tests)

SITE_BIT = 0x80000000


def edge_words(rows, cols, seed, step, site):
    """The four output words of every edge (rows[e] -> destination, cols[e] -> source): uint64 [nnz, 4]."""
    assert 0 <= site < SITE_BIT
    rows = np.asarray(rows, dtype=np.uint64)
    cols = np.asarray(cols, dtype=np.uint64)
    words = philox4x32_10([rows, cols, np.full_like(rows, step & 0xFFFFFFFF), np.full_like(rows, site | SITE_BIT)],
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return np.stack(words, axis=-1)


def keep_mask(rowptr, col, H, p, seed, step, site):
    """bool [nnz, H] over a CSR (self loops included, if the CSR has them), in CSR order."""
    assert 1 <= H <= 4 and 0.0 <= p < 1.0
    rowptr = np.asarray(rowptr, dtype=np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return edge_words(rows, col, seed, step, site)[:, :H] >= np.uint64(threshold(p))
