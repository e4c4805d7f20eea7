"""Contacts on the device (csrc/ensemble_contacts.hip) against the float64 numpy restatement of their definitions in tests/ref_contacts.py.

Every case here is a parity input: tests/test_ensemble_contacts_cpu.py asserts that its nearest comparison (a squared distance against a
squared cutoff or a squared bound (lam d0)^2) is at least 1e-9 relative from flipping, and both sides evaluate the same float64 expression,
a few 2^-53 apart at the most.  Contacts, counts, separation sums, the native list and the hits are therefore the same integers on both
sides and are held with ``==``.  What is left to a bound:

  P and the hard Q     one float64 division of two integers: BOUND = 4e-16, the bound the lDDT tests use for one division.
  d0                   a square root of the same v, correctly rounded or one ulp off: 2^-52 d0.
  the weighted map     the same R terms (w_r or 0.0) added in the same ascending order; if the device added them in another order or fused
                       an operation, each of its R - 1 additions could round differently, by 2^-53 of a partial sum <= the value: the bound is
                       (R + 2) 2^-52 max(1, value).
  the soft Q           SOFT_C = 16, bound (n + 16) 2^-52.  Q = (1 / n) sum of t_e, t = 1 / (1 + E), E = exp(x), x = beta (sqrt(v) - lam d0).
                       The kernel is built without contraction, so up to x both sides perform the same IEEE operations in the same order
                       (three exact differences of widened float32 values, three products, two additions, a correctly rounded square
                       root, the scaling lam d0, a subtraction, the scaling by beta): x is the same number.  From there: exp is within one
                       ulp on either side, so E differs by at most 2 ulp <= 2^-51 relative, which moves t by t (1 - t) 2^-51 <= 2^-53; the
                       addition 1 + E and the division each round once per side, 2^-53 t each: 4 * 2^-53.  One term differs by at most
                       5 * 2^-53 < 3 * 2^-52.  The two sides add the n terms, each in [0, 1], in different orders: either sum is within
                       (n - 1) 2^-53 of the exact sum relative, i.e. after the division by n within (n - 1) 2^-53 Q <= (n - 1) 2^-53 of
                       the exact mean, 2 (n - 1) 2^-53 between them, and the final division rounds once per side, 2^-52 together.
                       Total <= (n - 1 + 3 + 1) 2^-52 = (n + 3) 2^-52.  The plain count of one term's rounding operations -- three
                       differences, three squares, two additions, sqrt, two scalings, a subtraction, exp, add, divide = 15, at most 16
                       -- is the looser a-priori constant and the one asserted: (n + 16) 2^-52.
"""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import contact_cases as cases
import ref_contacts as ref
import ref_tm64
from conftest import GOLDEN, record_margin
from ensemble_cases import close_4 as _close_4, load_eval_entry, to_device as _dev, write_models

pytestmark = pytest.mark.gpu

BOUND = 4e-16
U52 = 2.0 ** -52
SOFT_C = 16


@functools.lru_cache(maxsize=None)
def reference(L, cutoff, sep):
    """The yardstick's outputs of one chain length and parameter set, computed once: the ensemble (with its two extreme structures), the
    counts, the statistics, the native list and Q."""
    a = cases.with_extremes(cases.ensembles(L)[0])
    a.setflags(write=False)
    pairs, d0 = ref.native_list(cases.native(L), cutoff, sep)
    out = {"a": a, "counts": ref.contact_counts(a, cutoff, sep), "stats": ref.contact_stats(a, cutoff, sep), "pairs": pairs, "d0": d0,
           "q": ref.native_q(a, pairs, d0)}
    for v in (out["counts"], pairs, d0, *out["stats"], *out["q"]):
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("cutoff,sep", cases.PARAMETERS)
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_contact_map_counts(L, cutoff, sep):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    want = reference(L, cutoff, sep)
    a = _dev(want["a"])
    counts, weighted = ops.ca_contact_map(a, cutoff, sep)
    assert weighted is None and counts.dtype == torch.int32 and counts.shape == (L, L)
    got = counts.cpu().numpy()
    assert (got == want["counts"]).all() and (got == got.T).all()
    band = np.abs(np.subtract.outer(np.arange(L), np.arange(L))) < sep
    assert (got[band] == 0).all()
    p = metrics.contact_map(want["a"], cutoff, sep)            # one division of the count by R
    assert p.dtype == np.float64 and (p == want["counts"] / float(len(want["a"]))).all()


@pytest.mark.parametrize("L", cases.WEIGHTED_LENGTHS)
def test_weighted_contact_map(L, monkeypatch):
    from str2str_amd import ops
    from str2str_amd.ops import ensemble

    a = cases.ensembles(L)[0]
    w = cases.weights(L)
    R = len(a)
    want = ref.weighted_map(a, w)
    da, dw = _dev(a), _dev(w)
    counts, weighted = ops.ca_contact_map(da, weights=dw)
    assert weighted.dtype == torch.float64 and weighted.shape == (L, L) and counts.dtype == torch.int32
    got = weighted.cpu().numpy()
    assert (counts.cpu().numpy() == ref.contact_counts(a)).all() and (got == got.T).all()
    err = float((np.abs(got - want) / np.maximum(1.0, want)).max())
    print(f"L={L} R={R}: max |weighted_gpu - weighted_ref| / max(1, value) = {err:.3e}")
    record_margin("ensemble_contact_map_weighted_rel", err, (R + 2) * U52)
    assert err <= (R + 2) * U52
    for chunk in (1, 7, R):                                    # launches over consecutive runs continue the one ascending sum
        monkeypatch.setattr(ensemble, "CONTACT_LAUNCH_STRUCTURES", chunk)
        c2, w2 = ops.ca_contact_map(da, weights=dw)
        assert torch.equal(w2, weighted) and torch.equal(c2, counts), chunk


def test_unweighted_chunks_and_splits(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.ops import ensemble

    for L in cases.WEIGHTED_LENGTHS:
        a = _dev(cases.ensembles(L)[0])
        whole = ops.ca_contact_map(a)[0]
        for chunk in (1, 7, a.shape[0]):
            monkeypatch.setattr(ensemble, "CONTACT_LAUNCH_STRUCTURES", chunk)
            assert torch.equal(ops.ca_contact_map(a)[0], whole), (L, chunk)
        monkeypatch.undo()
    # 601 x L = 16: one launch splits the structures over 38 workgroups of one batch each (the last is short); launches of 100 and of 16
    # structures split them otherwise
    s = ref_tm64.make_ensemble(np.random.default_rng(5), 601, 16, ref_tm64.random_walk(np.random.default_rng(6), 16))
    want = ref.contact_counts(s)
    big = ops.ca_contact_map(_dev(s))[0]
    assert (big.cpu().numpy() == want).all()
    for chunk in (100, 16):
        monkeypatch.setattr(ensemble, "CONTACT_LAUNCH_STRUCTURES", chunk)
        assert torch.equal(ops.ca_contact_map(_dev(s))[0], big), chunk
    n, sep_sum = ops.ca_contact_stats(_dev(s))                 # (still in launches of 16: tiles of 16 structures, one per launch)
    monkeypatch.undo()
    n2, sep_sum2 = ops.ca_contact_stats(_dev(s))
    assert torch.equal(n, n2) and torch.equal(sep_sum, sep_sum2)
    wn, ws = ref.contact_stats(s)
    assert (n.cpu().numpy() == wn).all() and (sep_sum.cpu().numpy() == ws).all()


@pytest.mark.parametrize("cutoff,sep", cases.PARAMETERS)
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_contact_stats(L, cutoff, sep):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    want = reference(L, cutoff, sep)
    n, sep_sum = ops.ca_contact_stats(_dev(want["a"]), cutoff, sep)
    assert n.dtype == torch.int32 and sep_sum.dtype == torch.int64 and n.shape == sep_sum.shape == (len(want["a"]),)
    wn, ws = want["stats"]
    assert (n.cpu().numpy() == wn).all() and (sep_sum.cpu().numpy() == ws).all()
    assert wn[-2] == 0 and (L > 31 or wn[-1] == max(0, L - sep) * (max(0, L - sep) + 1) // 2)   # the strand; the shrunk structure
    assert (wn.sum() == want["counts"].sum() // 2)
    rco = metrics.contact_order(want["a"], cutoff, sep)
    assert rco.dtype == np.float64 and np.abs(rco - ref.contact_order(wn, ws, L)).max() <= BOUND and rco[-2] == 0.0


@pytest.mark.parametrize("cutoff,sep", cases.PARAMETERS)
@pytest.mark.parametrize("L", cases.LENGTHS)
def test_native_list_and_q(L, cutoff, sep, monkeypatch):
    from str2str_amd import ops
    from str2str_amd.ops import ensemble

    want = reference(L, cutoff, sep)
    pairs, d0 = ops.ca_native_contacts(_dev(cases.native(L)), cutoff, sep)
    n = len(want["pairs"])
    assert pairs.dtype == torch.int32 and d0.dtype == torch.float64 and pairs.shape == (n, 2) and d0.shape == (n,)
    assert (pairs.cpu().numpy() == want["pairs"]).all()        # in order
    if n:
        err = float((np.abs(d0.cpu().numpy() - want["d0"]) / want["d0"]).max())
        record_margin("ensemble_native_d0_rel", err, U52)
        assert err <= U52
    a = _dev(want["a"])
    q_soft, q_hard, hits = ops.ca_native_q(a, pairs, d0)
    R = a.shape[0]
    assert q_soft.dtype == q_hard.dtype == torch.float64 and hits.dtype == torch.int32 and q_soft.shape == q_hard.shape == hits.shape == (R,)
    w_soft, w_hard, w_hits = want["q"]
    assert (hits.cpu().numpy() == w_hits).all()
    hard_err, soft_err = float(np.abs(q_hard.cpu().numpy() - w_hard).max()), float(np.abs(q_soft.cpu().numpy() - w_soft).max())
    print(f"L={L} cutoff={cutoff} sep={sep} n={n}: hard Q in [{w_hard.min():.3f}, {w_hard.max():.3f}], |soft_gpu - soft_ref| = {soft_err:.3e} "
          f"= {soft_err / U52:.2f} x 2^-52 (bound {n + SOFT_C})")
    record_margin("ensemble_q_hard_abs", hard_err, BOUND)
    record_margin("ensemble_q_soft_over_n_plus_c_ulp", soft_err / ((n + SOFT_C) * U52), 1.0)
    assert hard_err <= BOUND and soft_err <= (n + SOFT_C) * U52
    if L <= sep:
        assert n == 0
    if n == 0:                                                 # the empty list
        assert bool((q_soft == 1.0).all()) and bool((q_hard == 1.0).all()) and bool((hits == 0).all())
    for chunk in (1, 5):                                       # a structure's Q does not depend on the launch
        monkeypatch.setattr(ensemble, "CONTACT_LAUNCH_STRUCTURES", chunk)
        s2, h2, k2 = ops.ca_native_q(a, pairs, d0)
        assert torch.equal(s2, q_soft) and torch.equal(h2, q_hard) and torch.equal(k2, hits), chunk


def test_other_beta_and_lambda_and_nan():
    from str2str_amd import ops

    want = reference(65, 8.0, 3)
    a = np.array(want["a"][:6])
    pairs, d0 = _dev(want["pairs"]), _dev(want["d0"])
    n = len(want["pairs"])
    assert ref.margin(a, pairs=want["pairs"], d0=want["d0"], lam=1.5) >= ref.MARGIN
    w_soft, w_hard, w_hits = ref.native_q(a, want["pairs"], want["d0"], beta=2.0, lam=1.5)
    q_soft, q_hard, hits = ops.ca_native_q(_dev(a), pairs, d0, beta=2.0, lam=1.5)
    assert (hits.cpu().numpy() == w_hits).all() and np.abs(q_soft.cpu().numpy() - w_soft).max() <= (n + SOFT_C) * U52
    assert (w_hits != want["q"][2][:6]).any()
    a[1, 7] = np.nan                                           # a missing residue: its entries are not hit, its structure's soft Q is NaN
    w_soft, w_hard, w_hits = ref.native_q(a, want["pairs"], want["d0"])
    q_soft, q_hard, hits = ops.ca_native_q(_dev(a), pairs, d0)
    assert (hits.cpu().numpy() == w_hits).all() and bool(torch.isnan(q_soft[1])) and not bool(torch.isnan(q_soft[[0, 2, 3, 4, 5]]).any())
    counts = ops.ca_contact_map(_dev(a))[0].cpu().numpy()
    assert (counts == ref.contact_counts(a)).all()
    n_c, _ = ops.ca_contact_stats(_dev(a))
    assert (n_c.cpu().numpy() == ref.contact_stats(a)[0]).all()


def test_metrics_layer():
    from str2str_amd.metrics import metrics

    rng = np.random.default_rng(23)
    L = 22
    base = ref_tm64.random_walk(rng, L)
    target, pred = ref_tm64.make_ensemble(rng, 9, L, base), ref_tm64.make_ensemble(rng, 12, L, base, first_kind=1)
    both = {"target": target, "pred": pred}
    w = {"pred": np.random.default_rng(24).uniform(0.5, 2.0, size=12)}
    p_t, p_p = ref.contact_probability(target), ref.contact_probability(pred)
    assert (metrics.contact_map(pred) == p_p).all()
    got_w = metrics.contact_map(pred, weights=w["pred"])
    assert np.abs(got_w - ref.contact_probability(pred, weights=w["pred"])).max() <= 16 * U52
    iu = np.triu_indices(L, k=3)
    mae = metrics.contact_mae(both)
    assert mae["target"] == 0.0 and _close_4(mae["pred"], np.abs(p_p - p_t)[iu].mean())
    assert _close_4(metrics.contact_mae(both, weights=w)["pred"], np.abs(ref.contact_probability(pred, weights=w["pred"]) - p_t)[iu].mean())

    pairs, d0 = ref.native_list(target[0])
    g_pairs, g_d0 = metrics.native_contacts(target[0])
    assert g_pairs.dtype == np.int32 and (g_pairs == pairs).all() and np.abs(g_d0 - d0).max() <= U52 * d0.max()
    q_t, q_p = ref.native_q(target, pairs, d0), ref.native_q(pred, pairs, d0)
    n = len(pairs)
    got = metrics.fraction_native_contacts(pred, target[0])
    assert got.dtype == np.float64 and got.shape == (12,) and np.abs(got - q_p[0]).max() <= (n + SOFT_C) * U52
    assert np.abs(metrics.fraction_native_contacts(pred, target[0], soft=False) - q_p[1]).max() <= BOUND
    rco = metrics.contact_order(pred)
    assert np.abs(rco - ref.contact_order(*ref.contact_stats(pred), L)).max() <= BOUND

    mq = metrics.mean_q(both)
    assert _close_4(mq["target"], q_t[0].mean()) and _close_4(mq["pred"], q_p[0].mean())
    assert _close_4(metrics.mean_q(both, weights=w)["pred"], np.average(q_p[0], weights=w["pred"]))
    assert _close_4(metrics.mean_q(both, soft=False)["pred"], q_p[1].mean())
    js = metrics.js_q(both)
    h_t, h_p = (np.histogram(q, bins=50, range=(0.0, 1.0))[0] + metrics.PSEUDO_C for q in (q_t[0], q_p[0]))
    # (no Q of these ensembles lies within 1e-9 of a bin edge, so the histograms are the yardstick's)
    assert min(np.abs(q * 50 - np.round(q * 50)).min() for q in (q_t[0], q_p[0])) > 1e-9
    assert js["target"] == 0.0 and _close_4(js["pred"], metrics._js(h_p, h_t)) and js["pred"] > 0.0
    assert metrics.js_q({"target": target, "pred": target.copy()})["pred"] == 0.0
    # another native: the first structure of the other ensemble, as an explicit argument
    pairs2, d02 = ref.native_list(pred[0])
    assert ref.margin(target, pairs=pairs2, d0=d02) >= ref.MARGIN
    assert _close_4(metrics.mean_q(both, native=pred[0])["target"], ref.native_q(target, pairs2, d02)[0].mean())


def test_bad_arguments_raise_before_any_launch(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics
    from str2str_amd.ops import ensemble

    a = _dev(cases.ensembles(16)[0])
    pairs, d0 = ops.ca_native_contacts(a[0])

    def reached():
        raise AssertionError("reached the library")

    monkeypatch.setattr(ensemble, "load_library", reached)
    for call in (lambda: ops.ca_contact_map(a, cutoff=0.0), lambda: ops.ca_contact_map(a, min_seq_sep=0), lambda: ops.ca_contact_map(a[0]),
                 lambda: ops.ca_contact_map(a, weights=torch.ones(3, dtype=torch.float64, device="cuda")),
                 lambda: ops.ca_contact_map(a, weights=torch.ones(17, dtype=torch.float32, device="cuda")),
                 lambda: ops.ca_contact_map(a.double()), lambda: ops.ca_contact_stats(a, cutoff=float("nan")), lambda: ops.ca_contact_stats(a.cpu()),
                 lambda: ops.ca_native_contacts(a), lambda: ops.ca_native_contacts(a[0], min_seq_sep=0), lambda: ops.ca_native_q(a, pairs, d0, beta=0.0),
                 lambda: ops.ca_native_q(a, pairs, d0, lam=float("inf")), lambda: ops.ca_native_q(a, pairs.long(), d0),
                 lambda: ops.ca_native_q(a, pairs, d0.float()), lambda: ops.ca_native_q(a, pairs, d0[:-1]), lambda: ops.ca_native_q(a, pairs.cpu(), d0),
                 lambda: ops.ca_contact_map(torch.zeros(2, ops.CONTACT_MAX_RES + 1, 3, device="cuda"))):
        with pytest.raises(ops.HipLibraryError):
            call()
    x = cases.ensembles(16)[0]
    for call in (lambda: metrics.contact_map(x, weights=np.ones(3)), lambda: metrics.fraction_native_contacts(x, x[0][:15]),
                 lambda: metrics.fraction_native_contacts(x, x), lambda: metrics.mean_q({"target": x}, weights={"target": np.ones(2)})):
        with pytest.raises(ValueError):
            call()


def test_eval_contacts_switch(tmp_path):
    """The CLN025 fixture against an ensemble of noisy copies: with the switch the contacts csv (CONTACT_COLUMNS, a mean row) and the pair
    table hold what the metrics give for the files' coordinates; the metrics csv is byte for byte the one of a run without the switch,
    which writes no contacts file at all."""
    from str2str_amd.common.pdb_utils import extract_backbone_coords
    from str2str_amd.metrics import metrics

    entry = load_eval_entry("s2s_eval_entry_contacts")
    target_dir = os.path.join(GOLDEN, "pdb")
    template = os.path.join(target_dir, "CLN025.pdb")
    tgt = extract_backbone_coords(template)
    coords = tgt[0][None] + np.random.default_rng(3).normal(size=(6,) + tgt.shape[1:]) * 0.7
    listing = {}
    for sub, switch in (("plain", None), ("contacts", True)):
        pred_dir = tmp_path / sub / "samples" / "all"
        pred_dir.mkdir(parents=True)
        write_models(str(pred_dir / "CLN025.pdb"), template, coords)
        entry.evaluate_prediction(str(pred_dir), target_dir, tag="t", contacts=switch)
        files = glob.glob(str(tmp_path / sub / "metrics_t_*.csv"))
        assert len(files) == 1
        listing[sub] = (sorted(os.listdir(tmp_path / sub)), open(files[0], "rb").read())
    assert [f.split("_")[0] for f in listing["plain"][0]] == ["metrics", "samples"]          # no contacts* file without the switch
    assert [f.split("_")[0] for f in listing["contacts"][0]] == ["contacts", "contacts", "metrics", "samples"]
    assert listing["contacts"][1] == listing["plain"][1]
    rows = [ln.rstrip("\n").split("\t") for ln in open(glob.glob(str(tmp_path / "contacts" / "contacts_t_*.csv"))[0])]
    assert rows[0] == [""] + list(entry.CONTACT_COLUMNS) and [r[0] for r in rows[1:]] == ["CLN025", "mean"]
    ca = {"target": tgt, "pred": extract_backbone_coords(str(tmp_path / "contacts" / "samples" / "all" / "CLN025.pdb"))}
    q = metrics.mean_q(ca)
    want = [q["pred"], q["target"], metrics.js_q(ca)["pred"], metrics.contact_mae(ca)["pred"],
            np.around(metrics.contact_order(ca["pred"]).mean(), decimals=4), np.around(metrics.contact_order(ca["target"]).mean(), decimals=4)]
    assert [float(v) for v in rows[1][1:]] == [float(v) for v in want] and rows[2][1:] == rows[1][1:]
    assert 0.0 < want[0] <= 1.0 and 0.0 < want[1] <= 1.0
    assert os.listdir(tmp_path / "contacts" / "contacts") == ["CLN025.csv"]
    table = [ln.rstrip("\n").split("\t") for ln in open(tmp_path / "contacts" / "contacts" / "CLN025.csv")]
    assert table[0] == ["i", "j", "p_pred", "p_target"]
    p_pred, p_target = metrics.contact_map(ca["pred"]), metrics.contact_map(ca["target"])
    i, j = np.nonzero(np.triu((p_pred > 0) | (p_target > 0)))
    assert len(table) == 1 + len(i) > 1
    body = np.array([[float(v) for v in row] for row in table[1:]])
    assert (body[:, 0] == i).all() and (body[:, 1] == j).all() and (body[:, 1] - body[:, 0] >= 3).all()
    assert (body[:, 2] == np.around(p_pred[i, j], decimals=4)).all() and (body[:, 3] == np.around(p_target[i, j], decimals=4)).all()
