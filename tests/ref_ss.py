"""The yardstick of the secondary-structure kernel (csrc/ensemble_ss.hip): a vectorised float64 numpy statement of the definition in
include/str2str_hip.h -- Kabsch & Sander's hydrogen-bond energy, n-turns, bridges, ladders, bends and the state letters built from them,
with a threshold-only bond (no "two best bonds" bookkeeping) and no beta-bulge merging -- and of the backbone torsions phi, psi, omega.
tests/test_ensemble_ss_cpu.py holds it to constructed helices, to the fixture proteins' known anatomy and, for the dihedral, to the
reference through tests/golden/torsions.npz."""
import numpy as np

PRO = 14                                           # aatype in the reference's residue order
Q = 27.888                                         # 0.42 e x 0.20 e x 332 kcal A / mol
E_BOND, CA_REACH, R_MIN, E_MIN = -0.5, 9.0, 0.5, -9.9
COS_BEND = 0.3420201433256687                      # cos 70 degrees
MARGIN = 1e-9                                      # a device case keeps every comparison at least this far from flipping
LETTERS = "-BEHGITS"


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _len(v):
    return np.sqrt(_dot(v, v))


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def dihedral(p0, p1, p2, p3):
    """The IUPAC torsion of four points [..., 3] in radians, in (-pi, pi]: atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3))."""
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    n1, n2 = _cross(b1, b2), _cross(b2, b3)
    return np.arctan2(_len(b2) * _dot(b1, n2) + 0.0, _dot(n1, n2))


def connected(residue_index):
    """[L] bool: residue j follows residue j - 1 in the numbering."""
    ri = np.asarray(residue_index).astype(np.int64)
    c = np.zeros(len(ri), dtype=bool)
    c[1:] = ri[1:] == ri[:-1] + 1
    return c


def _unbroken(conn, a, b):
    """Ranges a .. b (arrays, a <= b, inside the chain) lie in one segment."""
    breaks = np.cumsum(~conn)
    return breaks[b] == breaks[a]


def _hydrogens(x, has_h):
    h = np.zeros((len(x), 3))
    co = x[:-1, 2] - x[:-1, 3]
    h[1:] = x[1:, 0] + co / _len(co)[:, None]
    return np.where(has_h[:, None], h, 0.0)


def _energies(x, aatype, ri):
    """-> E [L, L] (acceptor i, donor j), survivors [L, L] of the prefilter (j has H, j != i, j != i + 1, d(CA) < 9), d_CA, the four r."""
    L = len(x)
    conn = connected(ri)
    has_h = conn & (np.asarray(aatype) != PRO)
    h = _hydrogens(x, has_h)
    n, ca, c, o = x[:, 0], x[:, 1], x[:, 2], x[:, 3]
    d_ca = _len(ca[:, None] - ca[None, :])
    idx = np.arange(L)
    surv = has_h[None, :] & (idx[None, :] != idx[:, None]) & (idx[None, :] != idx[:, None] + 1) & (d_ca < CA_REACH)
    r = np.stack([_len(o[:, None] - n[None, :]), _len(c[:, None] - h[None, :]), _len(o[:, None] - h[None, :]), _len(c[:, None] - n[None, :])])
    with np.errstate(divide="ignore", invalid="ignore"):
        e = Q * (((1.0 / r[0] + 1.0 / r[1]) - 1.0 / r[2]) - 1.0 / r[3])
    e = np.where((r < R_MIN).any(0), E_MIN, e)
    return e, surv, d_ca, r


def _sh(m, di, dj):
    """m[i + di, j + dj], False outside."""
    L = len(m)
    out = np.zeros_like(m)
    i0, i1, j0, j1 = max(0, -di), min(L, L - di), max(0, -dj), min(L, L - dj)
    if i0 < i1 and j0 < j1:
        out[i0:i1, j0:j1] = m[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return out


def _bend_cos(x):
    """cos of the angle between CA_i - CA_i-2 and CA_i+2 - CA_i for 2 <= i <= L - 3 -> [L - 4] (empty for L < 5)."""
    ca = x[:, 1]
    u, v = ca[2:-2] - ca[:-4], ca[4:] - ca[2:-2]
    return _dot(u, v) / (_len(u) * _len(v))


def secondary_structure(atoms, aatype, residue_index):
    """One structure atoms [L, 5, 3] -> dict(ss 'S1' [L], n_hbonds int, hb_energy float64 [L], hb_partner int32 [L], hb bool [L, L],
    n_survivors int)."""
    x = np.asarray(atoms, dtype=np.float64)
    aatype, ri = np.asarray(aatype), np.asarray(residue_index).astype(np.int64)
    L = len(x)
    conn = connected(ri)
    e, surv, _, _ = _energies(x, aatype, ri)
    hb = surv & (e < E_BOND)
    masked = np.where(surv, e, np.inf)
    partner = np.where(surv.any(0), masked.argmin(0), -1).astype(np.int32)       # argmin: the lowest i among equals
    energy = np.where(partner >= 0, masked.min(0), 0.0)
    idx = np.arange(L)
    turn = {}
    for n in (3, 4, 5):
        t = np.zeros(L, dtype=bool)
        i = idx[:max(L - n, 0)]
        t[i] = _unbroken(conn, i, i + n) & hb[i, i + n]
        turn[n] = t
    ok3 = np.zeros(L, dtype=bool)
    if L >= 3:
        ok3[1:-1] = _unbroken(conn, idx[:-2], idx[2:])
    valid = ok3[:, None] & ok3[None, :] & (np.abs(idx[:, None] - idx[None, :]) >= 3)
    hbt = hb.T
    par = valid & ((_sh(hb, -1, 0) & _sh(hbt, 1, 0)) | (_sh(hbt, 0, -1) & _sh(hb, 0, 1)))
    anti = valid & ((hb & hbt) | (_sh(hb, -1, 1) & _sh(hbt, 1, -1)))
    bridge = (par | anti).any(1)
    ladder = ((par & (_sh(par, 1, 1) | _sh(par, -1, -1))) | (anti & (_sh(anti, 1, -1) | _sh(anti, -1, 1)))).any(1)
    bend = np.zeros(L, dtype=bool)
    if L >= 5:
        bend[2:-2] = _unbroken(conn, idx[:-4], idx[4:]) & (_bend_cos(x) < COS_BEND)
    ss = np.full(L, b"-", dtype="S1")
    ss[bridge] = b"B"
    ss[ladder] = b"E"

    def starts(n):                                             # i with turn_n(i - 1) and turn_n(i)
        s = np.zeros(L, dtype=bool)
        s[1:] = turn[n][:-1] & turn[n][1:]
        return np.nonzero(s)[0]

    for i in starts(4):
        ss[i:i + 4] = b"H"
    for n, letter in ((3, b"G"), (5, b"I")):
        before = ss.copy()
        for i in starts(n):
            if all(before[k] in (b"-", letter) for k in range(i, i + n)):
                ss[i:i + n] = letter
    for n in (3, 4, 5):
        for i in np.nonzero(turn[n])[0]:
            for k in range(i + 1, i + n):
                if ss[k] == b"-":
                    ss[k] = b"T"
    ss[bend & (ss == b"-")] = b"S"
    return dict(ss=ss, n_hbonds=int(hb.sum()), hb_energy=energy, hb_partner=partner, hb=hb, n_survivors=int(surv.sum()))


def torsions(atoms, residue_index):
    """One structure [L, 5, 3] -> (angles float64 [L, 3]: phi, psi, omega; mask bool [L, 3]); an undefined angle is 0.0."""
    x = np.asarray(atoms, dtype=np.float64)
    L = len(x)
    conn = connected(residue_index)
    ang, mask = np.zeros((L, 3)), np.zeros((L, 3), dtype=bool)
    if L >= 2:
        n, ca, c = x[:, 0], x[:, 1], x[:, 2]
        ang[1:, 0] = dihedral(c[:-1], n[1:], ca[1:], c[1:])
        ang[:-1, 1] = dihedral(n[:-1], ca[:-1], c[:-1], n[1:])
        ang[1:, 2] = dihedral(ca[:-1], c[:-1], n[1:], ca[1:])
        mask[1:, 0] = mask[1:, 2] = conn[1:]
        mask[:-1, 1] = conn[1:]
    return np.where(mask, ang, 0.0), mask


def ensemble(atoms, aatype, residue_index):
    """atoms [R, L, 5, 3] -> dict(ss 'S1' [R, L], n_hbonds int32 [R], hb_energy [R, L], hb_partner int32 [R, L], torsions [R, L, 3],
    torsion_mask [L, 3], n_survivors [R])."""
    per = [secondary_structure(x, aatype, residue_index) for x in atoms]
    out = {k: np.stack([np.asarray(p[k]) for p in per]) for k in ("ss", "hb_energy", "hb_partner", "n_survivors")}
    out["n_hbonds"] = np.array([p["n_hbonds"] for p in per], dtype=np.int32)
    tor = [torsions(x, residue_index) for x in atoms]
    out["torsions"], out["torsion_mask"] = np.stack([t[0] for t in tor]), tor[0][1]
    return out


def strings(ss):
    return ["".join(c.decode() for c in row) for row in np.atleast_2d(ss)]


def margin(atoms, aatype, residue_index):
    """The smallest distance of any comparison of the definition from flipping over the structures of atoms [R, L, 5, 3] (or one
    [L, 5, 3]): |E + 0.5| and |r - 0.5| over the prefilter's survivors, |d_CA - 9| over the pairs the other conditions leave, |cos - cos 70|
    over the bends of unbroken ranges.  inf when nothing is compared."""
    atoms = np.asarray(atoms, dtype=np.float64)
    aatype, ri = np.asarray(aatype), np.asarray(residue_index).astype(np.int64)
    conn = connected(ri)
    has_h = conn & (aatype != PRO)
    m = np.inf
    for x in atoms.reshape((-1,) + atoms.shape[-3:]):
        L = len(x)
        e, surv, d_ca, r = _energies(x, aatype, ri)
        idx = np.arange(L)
        tested = has_h[None, :] & (idx[None, :] != idx[:, None]) & (idx[None, :] != idx[:, None] + 1)
        if tested.any():
            m = min(m, float(np.abs(d_ca - CA_REACH)[tested].min()))
        if surv.any():
            m = min(m, float(np.abs(r - R_MIN)[:, surv].min()))
            far = surv & ~(r < R_MIN).any(0)
            if far.any():
                m = min(m, float(np.abs(e - E_BOND)[far].min()))
        if L >= 5:
            ok = _unbroken(conn, idx[:-4], idx[4:])
            if ok.any():
                m = min(m, float(np.abs(_bend_cos(x) - COS_BEND)[ok].min()))
    return m


def min_bond_sine(atoms, residue_index):
    """The smallest sine of a bond angle (p0 p1 p2 or p1 p2 p3) entering a defined torsion, over the structures; inf if there is none."""
    atoms = np.asarray(atoms, dtype=np.float64)
    conn = connected(residue_index)
    s = np.inf

    def sines(p0, p1, p2, p3, use):
        nonlocal s
        for a, b, c in ((p0, p1, p2), (p1, p2, p3)):
            u, v = a - b, c - b
            sin = _len(_cross(u, v)) / (_len(u) * _len(v))
            if use.any():
                s = min(s, float(sin[use].min()))

    for x in atoms.reshape((-1,) + atoms.shape[-3:]):
        if len(x) < 2:
            continue
        n, ca, c = x[:, 0], x[:, 1], x[:, 2]
        sines(c[:-1], n[1:], ca[1:], c[1:], conn[1:])
        sines(n[:-1], ca[:-1], c[:-1], n[1:], conn[1:])
        sines(ca[:-1], c[:-1], n[1:], ca[1:], conn[1:])
    return s


def propensity(ss):
    """ss 'S1' [R, L] -> float64 [L, 3]: the fractions of helix (H, G, I), strand (E, B) and other over the structures."""
    ss = np.atleast_2d(ss)
    helix, strand = np.isin(ss, [b"H", b"G", b"I"]), np.isin(ss, [b"E", b"B"])
    return np.stack([helix.mean(0), strand.mean(0), (~helix & ~strand).mean(0)], axis=1)
