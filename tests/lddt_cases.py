"""The inputs of the lDDT device tests, shared with the CPU test that asserts their margin (tests/test_ensemble_lddt_cpu.py): the recipe of
tests/ref_tm64.py -- exact copies, noisy copies, unrelated chains and mirror images around one random walk, each under its own rigid move."""
import functools

import numpy as np

import ref_tm64

# the empty set; one pair; the wave-width edges; several rows per lane of the list sweep; more than one block of list entries per thread;
# the narrow tile (above 425 residues); the cap
LENGTHS = (1, 2, 3, 5, 16, 31, 63, 64, 65, 130, 257, 400, 1024)
PER_RESIDUE_LENGTHS = (5, 64, 65, 257)
OTHER_PARAMETERS = (8.0, 3)          # (cutoff, min_seq_sep) of the second parameter set, at L = 65


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


@functools.lru_cache(maxsize=None)
def per_residue_inputs(L):
    """-> (model [9, L, 3], target [L, 3]) float32, read-only."""
    rng = np.random.default_rng(7000 + L)
    base = ref_tm64.random_walk(rng, L)
    model = ref_tm64.make_ensemble(rng, 9, L, base)
    target = np.asarray(ref_tm64.rigid_move(rng, base), dtype=np.float32)
    model.setflags(write=False); target.setflags(write=False)
    return model, target
