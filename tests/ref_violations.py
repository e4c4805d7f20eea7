"""The yardstick of the backbone violations (csrc/ensemble_violations.hip): a float64 numpy restatement of the definition in
include/str2str_hip.h -- the reference's between-residue bond, angle and clash terms and its extreme CA-CA steps (src/models/loss.py:714-1017,
1237-1314), restricted to N, CA, C, O, CB -- written from the formulas, one structure at a time.  tests/test_ensemble_violations_cpu.py holds
it to the reference's own functions through tests/golden/violations.npz and to cases worked by hand."""
import numpy as np

GLY, PRO = 7, 14                                   # aatype in the reference's residue order
RADIUS = np.array([1.55, 1.7, 1.7, 1.52, 1.7])     # N, CA, C, O, CB by element
CA_CA = 3.80209737096
MARGIN = 1e-10                                     # a device case keeps every comparison at least this far from flipping
LOSSES = ("c_n_loss_mean", "ca_c_n_loss_mean", "c_n_ca_loss_mean", "clashes_mean_loss")
FRACTIONS = ("violations_between_residue_bond", "violations_between_residue_clash", "violations_per_residue", "violations_extreme_ca_ca_distance")


def exists_from_aatype(aatype):
    """[L] -> [L, 5] bool: every backbone atom, and a CB except on GLY."""
    e = np.ones((len(aatype), 5), dtype=bool)
    e[np.asarray(aatype) == GLY, 4] = False
    return e


def _norm(v, eps):
    return np.sqrt(eps + ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]))


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _connections(x, exists, aatype, ri, tol):
    """-> per connection k -> k + 1: errors [3, L - 1], widths [3, L - 1] (tol x sigma), masks [3, L - 1], CA-CA excess and its mask."""
    eps = 1e-6
    ca0, c0, n1, ca1 = x[:-1, 1], x[:-1, 2], x[1:, 0], x[1:, 1]
    no_gap = (ri[1:] - ri[:-1]) == 1
    pro = aatype[1:] == PRO
    c_n = _norm(n1 - c0, eps)
    e_cn = np.sqrt(eps + (c_n - np.where(pro, 1.341, 1.329)) ** 2)
    u_ca, u_n, u_nca = (ca0 - c0) / _norm(ca0 - c0, eps)[:, None], (n1 - c0) / c_n[:, None], (ca1 - n1) / _norm(ca1 - n1, eps)[:, None]
    e_cacn = np.sqrt(eps + (_dot(u_ca, u_n) - -0.4473) ** 2)
    e_cnca = np.sqrt(eps + (_dot(-u_n, u_nca) - -0.5203) ** 2)
    # the widths as the reference has them: the CA-C-N cosine is held to the C-N LENGTH's 0.014 (loss.py:809), the C-N-CA cosine to 0.0353
    width = np.stack([tol * np.where(pro, 0.016, 0.014), np.full(len(pro), tol * 0.014), np.full(len(pro), tol * 0.0353)])
    m_cn = no_gap & exists[:-1, 2] & exists[1:, 0]
    mask = np.stack([m_cn, m_cn & exists[:-1, 1], m_cn & exists[1:, 1]])
    excess = _norm(ca0 - ca1, eps) - CA_CA
    return np.stack([e_cn, e_cacn, e_cnca]), width, mask, excess, no_gap & exists[:-1, 1] & exists[1:, 1]


def _atom_pairs(x, exists, ri, clash_tol):
    """-> d, bound, mask [L, L, 5, 5] over the ordered residue pairs (residue_index[i] < residue_index[j])."""
    dv = x[:, None, :, None, :] - x[None, :, None, :, :]
    d = _norm(dv, 1e-10)
    mask = exists[:, None, :, None] & exists[None, :, None, :] & (ri[:, None] < ri[None, :])[:, :, None, None]
    bonded = (ri[:, None] + 1) == ri[None, :]
    mask[:, :, 2, 0] &= ~bonded                    # C_i - N_i+1 is the peptide bond
    bound = np.broadcast_to((RADIUS[:, None] + RADIUS[None, :]) - clash_tol, d.shape)
    return d, bound, mask


def violations(atoms, atom_exists, aatype, residue_index, tolerance_factor=12.0, clash_tolerance=1.5):
    """One structure atoms [L, 5, 3] -> dict of the outputs of the definition (float64 / bool / int), and ``n_terms``: the number of summed
    terms behind every loss mean."""
    x = np.asarray(atoms, dtype=np.float64)
    exists, aatype, ri = np.asarray(atom_exists).astype(bool), np.asarray(aatype), np.asarray(residue_index).astype(np.int64)
    L = len(x)
    assert x.shape == (L, 5, 3) and exists.shape == (L, 5) and aatype.shape == (L,) and ri.shape == (L,)
    err, width, mask, excess, ca_mask = _connections(x, exists, aatype, ri, float(tolerance_factor))
    loss = np.maximum(err - width, 0.0)
    out = {name: float(np.sum(np.where(mask[q], loss[q], 0.0)) / (mask[q].sum() + 1e-6)) for q, name in enumerate(LOSSES[:3])}
    both = (loss[0] + loss[1]) + loss[2]           # (not masked: the reference's per_residue_loss_sum is not)
    out["per_residue_loss_sum"] = 0.5 * (np.append(both, 0.0) + np.append(0.0, both))
    violated = (mask & (err > width)).any(0)
    bond_mask = np.append(violated, False) | np.append(False, violated)
    d, bound, pair_mask = _atom_pairs(x, exists, ri, float(clash_tolerance))
    out["clashes_mean_loss"] = float(np.sum(np.where(pair_mask, np.maximum(bound - d, 0.0), 0.0)) / (1e-6 + pair_mask.sum()))
    clash = pair_mask & (d < bound)
    atom_mask = clash.any(axis=(1, 3)) | clash.any(axis=(0, 2))
    out.update(bond_mask=bond_mask, clash_atom_mask=atom_mask, n_clash_pairs=int(clash.sum()))
    res = 1e-4 + L
    out["violations_between_residue_bond"] = bond_mask.sum() / res
    out["violations_between_residue_clash"] = atom_mask.any(1).sum() / res
    out["violations_per_residue"] = (bond_mask | atom_mask.any(1)).sum() / res
    out["violations_extreme_ca_ca_distance"] = (ca_mask & (excess > 1.5)).sum() / (1e-4 + ca_mask.sum())
    out["n_terms"] = {LOSSES[0]: int(mask[0].sum()), LOSSES[1]: int(mask[1].sum()), LOSSES[2]: int(mask[2].sum()), LOSSES[3]: int(pair_mask.sum())}
    return out


def ensemble(atoms, atom_exists, aatype, residue_index, tolerance_factor=12.0, clash_tolerance=1.5):
    """atoms [R, L, 5, 3] -> the outputs of ``violations`` stacked over the structures (``n_terms`` is the sequence's: the first one's)."""
    per = [violations(x, atom_exists, aatype, residue_index, tolerance_factor, clash_tolerance) for x in atoms]
    out = {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0] if k != "n_terms"}
    out["n_terms"] = per[0]["n_terms"]
    return out


def margin(atoms, atom_exists, aatype, residue_index, tolerance_factor=12.0, clash_tolerance=1.5):
    """The smallest distance of any comparison of the definition from flipping, over the structures of atoms [R, L, 5, 3] (or one [L, 5, 3]):
    a counted atom pair's d against its bound (A), a counted connection error against its width, a counted CA-CA excess against 1.5.
    inf when nothing is compared.  (The prefilter is no comparison of the definition.)"""
    exists, aatype, ri = np.asarray(atom_exists).astype(bool), np.asarray(aatype), np.asarray(residue_index).astype(np.int64)
    atoms = np.asarray(atoms, dtype=np.float64)
    m = np.inf
    for x in atoms.reshape((-1,) + atoms.shape[-3:]):
        err, width, mask, excess, ca_mask = _connections(x, exists, aatype, ri, float(tolerance_factor))
        d, bound, pair_mask = _atom_pairs(x, exists, ri, float(clash_tolerance))
        for gap, use in ((np.abs(err - width), mask), (np.abs(excess - 1.5), ca_mask), (np.abs(d - bound), pair_mask)):
            if use.any():
                m = min(m, float(gap[use].min()))
    return m


def prefilter_survivors(atoms, atom_exists, residue_index, clash_tolerance=1.5):
    """(residue pairs i < j with different residue numbers that pass the kernel's CA prefilter, all such pairs) of one structure [L, 5, 3]:
    d(CA_i, CA_j) < rho_i + rho_j + (3.4 - clash_tolerance), rho = the largest distance of a residue's existing atoms from its CA."""
    x, exists, ri = np.asarray(atoms, dtype=np.float64), np.asarray(atom_exists).astype(bool), np.asarray(residue_index)
    rho = np.where(exists, np.sqrt(((x - x[:, 1:2]) ** 2).sum(-1)), 0.0)
    rho[:, 1] = 0.0
    rho = rho.max(1)
    d = np.sqrt(((x[:, None, 1] - x[None, :, 1]) ** 2).sum(-1))
    pairs = np.triu(ri[:, None] != ri[None, :], 1)
    return int((pairs & (d < rho[:, None] + rho[None, :] + (3.4 - clash_tolerance))).sum()), int(pairs.sum())
