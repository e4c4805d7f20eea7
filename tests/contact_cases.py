"""The inputs of the contact device tests, shared with the CPU test that asserts their margin (tests/test_ensemble_contacts_cpu.py): the
recipe of tests/lddt_cases.py -- exact copies, noisy copies, unrelated chains and mirror images around one random walk, each under its own
rigid move.  The ensemble ``a`` is mapped and scored, the first structure of ``b`` is the native."""
import functools

import numpy as np

import ref_tm64

# the empty sets (no eligible pair; no native contact); the first pair at each separation; the wave-width edges; several tiles of every
# tile size of the map; the cap
LENGTHS = (1, 2, 3, 4, 5, 16, 31, 63, 64, 65, 130, 257, 400, 1024)
PARAMETERS = ((8.0, 3), (10.0, 4))       # (cutoff, min_seq_sep)
WEIGHTED_LENGTHS = (5, 64, 65, 257)


def sizes(L):
    return (17, 24) if L < 130 else (5, 9) if L < 400 else (2, 3)


@functools.lru_cache(maxsize=None)
def ensembles(L):
    """-> (a [n_a, L, 3], b [n_b, L, 3]) float32, read-only."""
    rng = np.random.default_rng(6000 + L)
    base = ref_tm64.random_walk(rng, L)
    n_a, n_b = sizes(L)
    a, b = ref_tm64.make_ensemble(rng, n_a, L, base), ref_tm64.make_ensemble(rng, n_b, L, base, first_kind=3)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


def native(L):
    return ensembles(L)[1][0]


def with_extremes(a):
    """``a`` with two more structures: a straight strand of 3.4 A per residue (no contact: 10.2 A at separation 3, 13.6 A at 4) and the
    first structure shrunk to 0.15 (every eligible pair of a short chain is a contact)."""
    L = a.shape[1]
    strand = np.stack([np.zeros(L), np.zeros(L), 3.4 * np.arange(L)], axis=1).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([a, strand[None], a[:1] * np.float32(0.15)]))


def weights(L):
    """Random positive float64 weights, one per structure of ``a``."""
    return np.random.default_rng(8000 + L).uniform(0.1, 2.0, size=sizes(L)[0])
