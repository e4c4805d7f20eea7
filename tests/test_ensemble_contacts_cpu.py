"""The contact feature without a GPU: its yardstick (tests/ref_contacts.py) held to facts it did not produce -- an ideal alpha-helix, a
straight strand and mixtures of the two --, the margin that makes every device case a parity input, the host tails of the metrics, the
C-ABI surface, the evaluation switch and columns, and the argument checks that must fire before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import contact_cases as cases
import ref_contacts as ref
from conftest import ROOT

NAMES = ("s2s_ca_contact_map", "s2s_ca_contact_stats", "s2s_ca_native_contacts", "s2s_ca_native_q")


def helix(L):
    """An ideal alpha-helix CA trace: radius 2.3 A, 100 degrees and 1.5 A per residue.  |i - j| = 3, 4, 5 are 5.05, 6.20, 8.66 A apart."""
    k = np.arange(L)
    t = np.deg2rad(100.0) * k
    return np.stack([2.3 * np.cos(t), 2.3 * np.sin(t), 1.5 * k], axis=1).astype(np.float32)


def strand(L):
    """A straight strand, 3.4 A per residue: |i - j| = 3 is 10.2 A apart."""
    return np.stack([np.zeros(L), np.zeros(L), 3.4 * np.arange(L)], axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- the yardstick itself
@pytest.mark.parametrize("L", [8, 20, 33])
def test_helix_and_strand(L):
    h = helix(L)
    d = np.sqrt(ref.sq_dist(h))
    assert abs(d[0, 3] - 5.05) < 0.01 and abs(d[0, 4] - 6.20) < 0.01 and abs(d[0, 5] - 8.66) < 0.01
    c = ref.contacts(h)                                        # cutoff 8, separation 3: exactly (i, i + 3) and (i, i + 4)
    want = np.zeros((L, L), dtype=bool)
    i = np.arange(L)
    want[i[:-3], i[:-3] + 3] = True
    want[i[:-4], i[:-4] + 4] = True
    assert (c == want).all() and c.sum() == 2 * L - 7
    n, s = ref.contact_stats(np.stack([h, strand(L)]))
    assert n.dtype == np.int32 and s.dtype == np.int64
    assert n.tolist() == [2 * L - 7, 0] and s.tolist() == [3 * (L - 3) + 4 * (L - 4), 0]     # the strand has no contact
    rco = ref.contact_order(n, s, L)
    assert rco[0] == (3 * (L - 3) + 4 * (L - 4)) / (L * (2 * L - 7)) and rco[1] == 0.0
    counts = ref.contact_counts(np.stack([h, strand(L)]))
    assert counts.dtype == np.int32 and (counts == counts.T).all() and (counts == (want | want.T)).all()


def test_mixture_of_helices_and_strands():
    L, n_h, n_e = 20, 5, 3
    ens = np.stack([helix(L)] * n_h + [strand(L)] * n_e)[[0, 5, 1, 6, 2, 7, 3, 4]]       # interleaved
    is_helix = np.array([1, 0, 1, 0, 1, 0, 1, 1], dtype=bool)
    p = ref.contact_probability(ens)
    assert p[2, 5] == p[5, 2] == n_h / (n_h + n_e) and p[2, 6] == n_h / (n_h + n_e) and p[2, 7] == 0.0 and p[2, 4] == 0.0
    w = np.random.default_rng(3).uniform(0.5, 2.0, size=len(ens))
    pw = ref.contact_probability(ens, weights=w)
    assert abs(pw[2, 5] - w[is_helix].sum() / w.sum()) <= 4 * 2.0 ** -52 and pw[2, 7] == 0.0
    acc = 0.0                                                  # the weighted numerator is the explicit ascending sum
    for r in range(len(ens)):
        acc = acc + (w[r] if is_helix[r] else 0.0)
    assert ref.weighted_map(ens, w)[2, 5] == acc
    pairs, d0 = ref.native_list(helix(L))                      # cutoff 8, separation 4: the (i, i + 4) alone
    assert pairs.tolist() == [[i, i + 4] for i in range(L - 4)] and np.abs(d0 - 6.20).max() < 0.01
    q_soft, q_hard, hits = ref.native_q(ens, pairs, d0)
    assert (q_hard == is_helix).all() and (hits == np.where(is_helix, L - 4, 0)).all()    # 13.6 A on the strand against 1.2 x 6.2
    assert (q_soft[is_helix] > 0.99).all() and (q_soft[~is_helix] < 1e-10).all()


def test_soft_q_of_a_structure_against_itself_is_the_closed_form():
    x = cases.ensembles(65)[0][2]
    pairs, d0 = ref.native_list(x)
    assert len(pairs) > 100
    q_soft, q_hard, hits = ref.native_q(x[None], pairs, d0)
    want = np.mean(1.0 / (1.0 + np.exp(-ref.BETA * (ref.LAM - 1.0) * d0)))
    assert abs(q_soft[0] - want) <= 64 * 2.0 ** -52 and q_soft[0] < 1.0 and q_hard[0] == 1.0 and hits[0] == len(pairs)


def test_min_seq_sep_nan_and_the_empty_list():
    x = cases.ensembles(16)[0][0].copy()
    for sep in (1, 2, 3, 7, 15, 16, 40):
        c = ref.contacts(x, 100.0, sep)                        # a cutoff nothing exceeds: exactly the eligible pairs
        assert c.sum() == max(0, 16 - sep) * (max(0, 16 - sep) + 1) // 2 and not np.tril(c, sep - 1).any()
    full = ref.contacts(x, 8.0, 3)
    x[5] = np.nan
    c = ref.contacts(x, 8.0, 3)
    assert not c[5].any() and not c[:, 5].any() and (np.delete(np.delete(c, 5, 0), 5, 1) == np.delete(np.delete(full, 5, 0), 5, 1)).all()
    pairs, d0 = ref.native_list(cases.ensembles(16)[0][0], 8.0, 3)
    q_soft, q_hard, hits = ref.native_q(x[None], pairs, d0)    # a NaN residue misses its hits and makes the soft Q NaN
    assert hits[0] == len(pairs) - int(((pairs == 5).any(1)).sum()) and np.isnan(q_soft[0])
    for L in (1, 2, 3, 4):                                     # no pair is 4 apart: n = 0 gives 1.0
        a, _ = cases.ensembles(L)
        pairs, d0 = ref.native_list(cases.native(L))
        assert pairs.shape == (0, 2) and d0.shape == (0,)
        q_soft, q_hard, hits = ref.native_q(a, pairs, d0)
        assert (q_soft == 1.0).all() and (q_hard == 1.0).all() and (hits == 0).all()
    assert ref.margin(cases.ensembles(2)[0]) == np.inf


def test_margin_sees_a_pair_on_the_edge():
    x = np.zeros((1, 4, 3), dtype=np.float32)
    x[0, :, 0] = [0.0, 100.0, 200.0, 8.0 * (1.0 - 1e-4)]     # the one eligible pair (0, 3) sits 1e-4 relative inside the cutoff
    assert abs(ref.margin(x, 8.0, 3) - 2e-4) < 1e-6          # (in squared form: twice)
    pairs, d0 = np.array([[0, 3]], dtype=np.int32), np.array([8.0 / 1.2])
    assert abs(ref.margin(x, pairs=pairs, d0=d0) - 2e-4) < 1e-6


# --------------------------------------------------------------------------------------------------------- the device cases' margin
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_every_device_case_is_a_parity_input(L):
    """The device compares the same float64 v with the same squared bounds; a fused multiply-add or a bound squared another way moves
    either by a few 2^-53 relative.  A case whose nearest comparison is >= 1e-9 relative from flipping has identical integers on both
    sides.  A condition on the cases; none is left out."""
    a, _ = cases.ensembles(L)
    nat = cases.native(L)
    for cutoff, sep in cases.PARAMETERS:
        pairs, d0 = ref.native_list(nat, cutoff, sep)
        full = cases.with_extremes(a)
        m = min(ref.margin(full, cutoff, sep), ref.margin(nat[None], cutoff, sep), ref.margin(full, pairs=pairs, d0=d0))
        print(f"L={L} cutoff={cutoff} sep={sep}: margin {m:.3e}, |list| = {len(pairs)}")
        assert m >= ref.MARGIN, m
    for cutoff, sep in cases.PARAMETERS:
        n, _ = ref.contact_stats(cases.with_extremes(a), cutoff, sep)
        assert n[-2] == 0                                      # the strand has no contact
        if L <= 31:                                            # the shrunk structure is all contacts while the chain is short enough
            assert n[-1] == max(0, L - sep) * (max(0, L - sep) + 1) // 2


def test_the_other_device_inputs_are_parity_inputs():
    import ref_tm64

    s = ref_tm64.make_ensemble(np.random.default_rng(5), 601, 16, ref_tm64.random_walk(np.random.default_rng(6), 16))
    assert ref.margin(s) >= ref.MARGIN
    a = cases.ensembles(65)[0][:6]                             # the second (beta, lam) of the device test
    pairs, d0 = ref.native_list(cases.native(65), 8.0, 3)
    assert ref.margin(a, pairs=pairs, d0=d0, lam=1.5) >= ref.MARGIN
    for L in cases.WEIGHTED_LENGTHS:
        assert ref.margin(cases.ensembles(L)[0]) >= ref.MARGIN and (cases.weights(L) > 0).all()
    rng = np.random.default_rng(23)
    base = ref_tm64.random_walk(rng, 22)
    target, pred = ref_tm64.make_ensemble(rng, 9, 22, base), ref_tm64.make_ensemble(rng, 12, 22, base, first_kind=1)
    pairs, d0 = ref.native_list(target[0])
    assert min(ref.margin(target), ref.margin(pred), ref.margin(target[:1], 8.0, 4), ref.margin(target, pairs=pairs, d0=d0),
               ref.margin(pred, pairs=pairs, d0=d0)) >= ref.MARGIN


# ------------------------------------------------------------------------------------------------------- the metrics' host tails
def test_metric_tails_on_the_yardstick(monkeypatch):
    """contact_mae, js_q and mean_q finish on the host: with the two device-backed functions they build on replaced by the yardstick,
    an ensemble against itself is 0.0 and two different ones give the plain numpy values."""
    from str2str_amd.metrics import metrics

    monkeypatch.setattr(metrics, "contact_map", lambda v, cutoff=8.0, min_seq_sep=3, weights=None: ref.contact_probability(np.asarray(v), cutoff, min_seq_sep, weights))
    monkeypatch.setattr(metrics, "fraction_native_contacts",
                        lambda v, native, soft=True, beta=5.0, lam=1.2, cutoff=8.0, min_seq_sep=4:
                        ref.native_q(np.asarray(v), *ref.native_list(np.asarray(native), cutoff, min_seq_sep), beta, lam)[0 if soft else 1])
    a, b = cases.ensembles(31)
    both = {"target": a, "pred": b, "same": a.copy()}
    mae = metrics.contact_mae(both)
    assert mae["target"] == 0.0 and mae["same"] == 0.0 and mae["pred"] > 0.0
    iu = np.triu_indices(31, k=3)
    assert mae["pred"] == np.around(np.abs(ref.contact_probability(b) - ref.contact_probability(a))[iu].mean(), decimals=4)
    js = metrics.js_q(both)
    assert js["target"] == 0.0 and js["same"] == 0.0 and 0.0 < js["pred"] <= 1.0
    pairs, d0 = ref.native_list(a[0])
    qa, qb = ref.native_q(a, pairs, d0)[0], ref.native_q(b, pairs, d0)[0]
    ha, hb = (np.histogram(q, bins=50, range=(0.0, 1.0))[0] + metrics.PSEUDO_C for q in (qa, qb))
    assert js["pred"] == np.around(metrics._js(hb, ha), decimals=4)
    mq = metrics.mean_q(both)
    assert mq["target"] == mq["same"] == np.around(qa.mean(), decimals=4) and mq["pred"] == np.around(qb.mean(), decimals=4)
    w = {"pred": np.random.default_rng(4).uniform(0.5, 2.0, size=len(b))}
    assert metrics.mean_q(both, weights=w)["pred"] == np.around(np.average(qb, weights=w["pred"]), decimals=4)
    hard = metrics.mean_q(both, native=b[0], soft=False, cutoff=10.0)
    pairs, d0 = ref.native_list(b[0], 10.0, 4)
    assert hard["pred"] == np.around(ref.native_q(b, pairs, d0)[1].mean(), decimals=4)
    assert metrics.contact_mae({"target": a[:, :2], "pred": b[:, :2]}) == {"pred": 0.0, "target": 0.0}   # no pair 3 apart


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_header_declares_and_ops_exports_the_entry_points():
    from str2str_amd import ops
    from str2str_amd.ops import binding, ensemble

    text = open(os.path.join(ROOT, "include", "str2str_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"^int\s+(s2s_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M))
    for name in NAMES:
        assert name in protos and name in ops.EXPORTS
        args = [a.strip() for a in protos[name].split(",")]
        assert args[-1] == "void* stream" and len(args) == len(binding._SIGNATURES[name])
    assert int(re.search(r"#define\s+S2S_CONTACT_MAX_RES\s+(\d+)", hdr).group(1)) == ops.CONTACT_MAX_RES == ensemble.CONTACT_MAX_RES == 1024
    assert int(re.search(r"#define\s+S2S_CONTACT_MAX_STRUCTURES\s+(\d+)", hdr).group(1)) == ensemble.CONTACT_LAUNCH_STRUCTURES == 65535
    assert ops.ABI_VERSION == 40
    assert int(re.search(r"return (\d+);", open(os.path.join(ROOT, "str2str_amd", "csrc", "abi.hip")).read()).group(1)) == 40
    for fn in (ops.ca_contact_map, ops.ca_contact_stats, ops.ca_native_contacts, ops.ca_native_q):
        assert callable(fn)
    for said in ("CA atoms only", "BELOW 1", "lam = 1.2", "Best, Hummer and Eaton", "ascending"):   # what the header owes its reader
        assert said in text


def test_bad_sizes_are_invalid_value():
    """Sizes and parameters the kernels cannot take are rejected before any launch (hipErrorInvalidValue = 1), so this needs no device."""
    from str2str_amd import build, ops

    if not os.path.exists(ops.LIB_PATH):
        build.build(verbose=False)
    lib = ops.load_library()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf, cap = float("nan"), float("inf"), ops.CONTACT_MAX_RES
    for n, L, cutoff, sep in ((0, 8, 8.0, 3), (4, 0, 8.0, 3), (4, cap + 1, 8.0, 3), (4, 8, 0.0, 3), (4, 8, -1.0, 3), (4, 8, nan, 3),
                              (4, 8, inf, 3), (4, 8, 8.0, 0), (4, 8, 8.0, -2)):
        assert lib.s2s_ca_contact_map(p, n, L, cutoff, sep, None, p, None, None) == 1, (n, L, cutoff, sep)
        assert lib.s2s_ca_contact_stats(p, n, L, cutoff, sep, p, p, None) == 1, (n, L, cutoff, sep)
        if n:
            assert lib.s2s_ca_native_contacts(p, L, cutoff, sep, p, p, p, None) == 1, (L, cutoff, sep)
    assert lib.s2s_ca_contact_map(p, 65536, 8, 8.0, 3, None, p, None, None) == 1
    for args in ((None, 4, 8, 8.0, 3, None, p, None), (p, 4, 8, 8.0, 3, None, None, None), (p, 4, 8, 8.0, 3, p, p, None),
                 (p, 4, 8, 8.0, 3, None, p, p)):               # a missing buffer; weights without their sums and the reverse
        assert lib.s2s_ca_contact_map(*args, None) == 1
    for args in ((None, 4, 8, 8.0, 3, p, p), (p, 4, 8, 8.0, 3, None, p), (p, 4, 8, 8.0, 3, p, None)):
        assert lib.s2s_ca_contact_stats(*args, None) == 1
    for args in ((None, 8, 8.0, 3, p, p, p), (p, 8, 8.0, 3, None, p, p), (p, 8, 8.0, 3, p, None, p), (p, 8, 8.0, 3, p, p, None)):
        assert lib.s2s_ca_native_contacts(*args, None) == 1
    for n, L, n_pairs, beta, lam in ((0, 8, 5, 5.0, 1.2), (4, 0, 5, 5.0, 1.2), (4, cap + 1, 5, 5.0, 1.2), (4, 8, -1, 5.0, 1.2), (4, 8, 29, 5.0, 1.2),
                                     (4, 8, 5, 0.0, 1.2), (4, 8, 5, nan, 1.2), (4, 8, 5, inf, 1.2), (4, 8, 5, 5.0, 0.0), (4, 8, 5, 5.0, -1.0),
                                     (4, 8, 5, 5.0, nan)):
        assert lib.s2s_ca_native_q(p, n, L, p, p, n_pairs, beta, lam, p, p, p, None) == 1, (n, L, n_pairs, beta, lam)
    for args in ((None, 4, 8, p, p, 5, 5.0, 1.2, p, p, p), (p, 4, 8, None, p, 5, 5.0, 1.2, p, p, p), (p, 4, 8, p, None, 5, 5.0, 1.2, p, p, p),
                 (p, 4, 8, p, p, 5, 5.0, 1.2, None, p, p), (p, 4, 8, p, p, 5, 5.0, 1.2, p, None, p), (p, 4, 8, p, p, 5, 5.0, 1.2, p, p, None)):
        assert lib.s2s_ca_native_q(*args, None) == 1


def test_argument_checks_fire_before_the_device(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics
    from str2str_amd.ops import ensemble

    def touched(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(ensemble, "load_library", touched)
    x = torch.zeros(4, 8, 3)
    shapes = [(dict(ca=torch.zeros(4, 8)), "coordinates"), (dict(ca=torch.zeros(4, 8, 2)), "coordinates"), (dict(ca=torch.zeros(0, 8, 3)), "coordinates"),
              (dict(ca=torch.zeros(4, 0, 3)), "coordinates"), (dict(ca=np.zeros((4, 8, 3), dtype=np.float32)), "tensors"),
              (dict(ca=torch.zeros(2, ops.CONTACT_MAX_RES + 1, 3)), "residues"), (dict(ca=x), "no CPU fallback")]
    cut = [(dict(ca=x, cutoff=0.0), "cutoff"), (dict(ca=x, cutoff=float("nan")), "cutoff"), (dict(ca=x, cutoff=float("inf")), "cutoff"),
           (dict(ca=x, min_seq_sep=0), "min_seq_sep"), (dict(ca=x, min_seq_sep=1.5), "min_seq_sep"), (dict(ca=x, min_seq_sep=True), "min_seq_sep")]
    for fn in (ops.ca_contact_map, ops.ca_contact_stats):
        for kwargs, match in shapes + cut:
            with pytest.raises(ops.HipLibraryError, match=match):
                fn(**kwargs)
    for w in (torch.zeros(3, dtype=torch.float64), torch.zeros(4, 1, dtype=torch.float64), [1.0] * 4):
        with pytest.raises(ops.HipLibraryError, match="weights"):
            ops.ca_contact_map(x, weights=w)
    for native in (torch.zeros(4, 8, 3), torch.zeros(8), torch.zeros(8, 2), torch.zeros(0, 3), np.zeros((8, 3)), torch.zeros(ops.CONTACT_MAX_RES + 1, 3),
                   torch.zeros(8, 3)):
        with pytest.raises(ops.HipLibraryError):
            ops.ca_native_contacts(native)
    for kwargs, match in cut:
        with pytest.raises(ops.HipLibraryError, match=match):
            ops.ca_native_contacts(torch.zeros(8, 3), **{k: v for k, v in kwargs.items() if k != "ca"})
    pairs, d0 = torch.zeros(5, 2, dtype=torch.int32), torch.zeros(5, dtype=torch.float64)
    for kwargs, match in shapes:
        with pytest.raises(ops.HipLibraryError, match=match):
            ops.ca_native_q(kwargs["ca"], pairs, d0)
    for kwargs, match in ((dict(beta=0.0), "beta"), (dict(beta=float("nan")), "beta"), (dict(lam=-1.2), "lam"), (dict(lam=float("inf")), "lam")):
        with pytest.raises(ops.HipLibraryError, match=match):
            ops.ca_native_q(x, pairs, d0, **kwargs)
    for bad_pairs, bad_d0 in ((torch.zeros(5, 3, dtype=torch.int32), d0), (pairs, torch.zeros(4, dtype=torch.float64)), (pairs.numpy(), d0),
                              (torch.zeros(29, 2, dtype=torch.int32), torch.zeros(29, dtype=torch.float64))):     # 28 pairs exist at L = 8
        with pytest.raises(ops.HipLibraryError):
            ops.ca_native_q(x, bad_pairs, bad_d0)

    # the metrics reach the device through _dev only
    monkeypatch.setattr(metrics, "_dev", touched)
    with pytest.raises(ValueError, match="weights"):
        metrics.contact_map(np.zeros((4, 8, 3)), weights=np.ones(3))
    with pytest.raises(ValueError, match="weights"):
        metrics.js_q({"target": np.zeros((4, 8, 3))}, weights={"target": np.ones(5)})
    for call in (lambda: metrics.native_contacts(np.zeros((2, 8, 3))), lambda: metrics.fraction_native_contacts(np.zeros((4, 8, 3)), np.zeros((1, 8, 3)))):
        with pytest.raises(ValueError, match="native"):
            call()
