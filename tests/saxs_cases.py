"""The deterministic inputs of the solution-scattering tests, shared by the CPU test and the device test: the CA traces of the ensembles of
``ss_cases`` (helices, mixed chains, strands, pi-helices and the COMPACT members shrunk to 0.15) under several q-lists and form-factor
tables.  The yardstick's result of a case is computed once (``reference``) and shared read-only."""
import functools
from typing import NamedTuple, Optional

import numpy as np

import ref_saxs as ref
import ss_cases

# (L, R): one bead (no pair); one pair; fewer pairs than a wave; general cases; 253 and 276 pairs, on either side of the 256-thread stride;
# several strides with a ragged last one; a chain above 256 residues, where every row of the triangle is first longer, then shorter than
# the stride
SHAPES = ((1, 2), (2, 1), (3, 4), (13, 17), (23, 3), (24, 3), (31, 9), (64, 3), (65, 17), (257, 2))
LONG = (1024, 1)                   # the cap: 523 776 pairs, at LONG_Q
LONG_Q = (0.0, 0.1, 0.6)
# 0.0 (every sinc is 1.0 by rule), a duplicate, and 0.6 (the largest argument: a up to 58 at 257 residues)
Q_DEFAULT = (0.0, 0.013, 0.05, 0.05, 0.21, 0.6)
N_Q = (1, 15, 16, 17, 33)          # on (31, 9): one q; one short of a tile, a tile, one past it; two tiles and one q
MANY_Q = (13, 2, 1024)             # (L, R, n_q): S2S_SAXS_MAX_Q, 64 tiles
N_TYPES = (1, 3, 21)               # on (31, 9) and (65, 17)


class Case(NamedTuple):
    ca: np.ndarray                 # float32 [R, L, 3]
    q: np.ndarray                  # float64 [Q]
    types: Optional[np.ndarray]    # int32 [L], None: the default (all 0)
    table: Optional[np.ndarray]    # float64 [n_types, Q], None: the default (one type, all ones)
    aatype: np.ndarray             # [L], the generator's sequence


def tags():
    return ([f"L{L}_R{R}" for L, R in SHAPES] + [f"L{LONG[0]}_R{LONG[1]}_long"] + [f"L31_R9_Q{n}" for n in N_Q]
            + ["L{}_R{}_Q{}".format(*MANY_Q)] + [f"L{L}_R{R}_T{n}" for L, R in ((31, 9), (65, 17)) for n in N_TYPES])


@functools.lru_cache(maxsize=None)
def ca_ensemble(L, R):
    """-> (CA [R, L, 3] float32, aatype [L]) of ``ss_cases.ensemble(L, R)``, read-only."""
    atoms, aatype, _ = ss_cases.ensemble(L, R)
    ca = np.ascontiguousarray(atoms[:, :, 1])
    ca.setflags(write=False)
    return ca, aatype


def q_list(n):
    """n q-values in [0, 0.6]: random, with 0.0, a duplicate and 0.6 among them from four values on."""
    q = np.random.default_rng(77000 + n).uniform(0.001, 0.6, size=n)
    if n >= 4:
        q[1], q[n // 2], q[n - 1] = 0.0, q[0], 0.6
    return q


def form_factors(n_types, L, aatype, q):
    """-> (types int32 [L], table [n_types, Q]): values around 1 with the whole column of q index 1 negative and, from three types on,
    the whole row of type 1 (negative contrast); every type occurs where the chain is long enough."""
    rng = np.random.default_rng(88000 + n_types)
    table = 1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=(n_types, len(q)))
    if n_types >= 3:
        table[1] *= -1.0
    if len(q) > 1:
        table[:, 1] = -np.abs(table[:, 1])
    types = (np.asarray(aatype) % n_types).astype(np.int32)
    types[:min(L, n_types)] = np.arange(min(L, n_types))[::-1]
    return types, table


@functools.lru_cache(maxsize=None)
def case(tag) -> Case:
    parts = tag.split("_")
    L, R = int(parts[0][1:]), int(parts[1][1:])
    ca, aatype = ca_ensemble(L, R)
    q, types, table = np.asarray(Q_DEFAULT), None, None
    rest = parts[2] if len(parts) > 2 else ""
    if rest == "long":
        q = np.asarray(LONG_Q)
    elif rest.startswith("Q"):
        q = q_list(int(rest[1:]))
    elif rest.startswith("T"):
        types, table = form_factors(int(rest[1:]), L, aatype, q)
    elif rest:
        raise KeyError(tag)
    for a in (q, types, table):
        if a is not None:
            a.setflags(write=False)
    return Case(ca, q, types, table, aatype)


@functools.lru_cache(maxsize=None)
def reference(tag):
    """The yardstick's (intensity [R, Q], inv_r_mean [R]) of a case, read-only."""
    c = case(tag)
    want = ref.scattering(c.ca, c.q, c.types, c.table)
    for v in want:
        v.setflags(write=False)
    return want


def amplitude_sq(c: Case):
    """(sum_i |f_i(q_k)|)^2 per q-value [Q]: the scale of the device test's bound."""
    L = c.ca.shape[1]
    f = np.ones((L, len(c.q))) if c.table is None else c.table[c.types]
    return np.abs(f).sum(axis=0) ** 2
