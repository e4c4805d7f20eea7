"""The host side of the per-structure metrics, without a device: the switches and columns of eval.py's optional reports, the value-level
summaries of str2str_amd.metrics against their restatement in plain numpy, and the argument checks every ensemble wrapper shares."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from ensemble_cases import load_eval_entry

EXTRA_METRICS = ("val_bb_bond", "val_bb_clash", "viol_per_residue", "div_rmsd", "rmsd_recall", "rmsd_precision", "div_tm", "tm_recall",
                 "tm_precision", "div_lddt", "lddt_recall", "lddt_precision")
REPORT_COLUMNS = {"secondary_structure": ("SS_COLUMNS", ("ss_helix", "ss_strand", "ss_helix_target", "ss_strand_target", "ss_mae", "js_rama")),
                  "contacts": ("CONTACT_COLUMNS", ("q_mean", "q_mean_target", "js_q", "contact_mae", "rco", "rco_target")),
                  "sasa": ("SASA_COLUMNS", ("sasa_mean", "sasa_mean_target", "js_sasa", "sasa_mae")),
                  "saxs": ("SAXS_COLUMNS", ("saxs_mae", "rh_mean", "rh_mean_target", "js_rh"))}


# ---------------------------------------------------------------------------------------------------------------------- eval.py
@pytest.mark.parametrize("name", list(REPORT_COLUMNS))
def test_report_columns_and_the_switch(name, monkeypatch):
    from str2str_amd.utils import config as C

    entry = load_eval_entry(f"s2s_eval_entry_{name}_cpu")
    attr, columns = REPORT_COLUMNS[name]
    switch = getattr(entry, f"{name}_switch")
    assert getattr(entry, attr) == columns and entry.SS_CLASSES == ("helix", "strand", "other")
    assert entry.EXTRA_METRICS == EXTRA_METRICS and len(entry.EXTRA_METRICS) == 12 and len(entry.BACKBONE_METRICS) == 3
    others = set(entry.EXTRA_METRICS) | set(entry.CLUSTER_COLUMNS) | set(entry.metric_columns(None))
    for other, (other_attr, _) in REPORT_COLUMNS.items():
        if other != name:
            others |= set(getattr(entry, other_attr))
    assert not (set(columns) | ({"saxs_chi2"} if name == "saxs" else set())) & others
    monkeypatch.setenv("TEST_DATA", "/nonexistent")
    compose = lambda *args: C.compose(os.path.join(ROOT, "configs"), "eval.yaml", list(args))   # noqa: E731
    assert switch(compose(f"+{name}=true").get(name)) is True
    assert switch(compose(f"+{name}=false").get(name)) is False
    assert compose().get(name) is None and compose().get("saxs_data") is None
    assert compose("+saxs=true", "+saxs_data=/some/dir").get("saxs_data") == "/some/dir"
    for value, want in ((None, False), (True, True), (False, False), ("true", True), ("false", False), ("False", False), (" True ", True),
                        ("0", False), ("yes", True)):
        assert switch(value) is want
    for bad in ("maybe", 2, 1.0, 2.5, [True]):
        with pytest.raises(ValueError, match=name):
            switch(bad)
    with pytest.raises(ValueError, match=name):                 # rejected before anything is read or written
        entry.evaluate_prediction("/nonexistent/pred", "/nonexistent/target", **{name: "maybe"})
    with pytest.raises(ValueError, match="saxs_data"):
        entry.evaluate_prediction("/nonexistent/pred", "/nonexistent/target", saxs_data="/some/dir", **({} if name == "saxs" else {name: True}))
    params = inspect.signature(entry.evaluate_prediction).parameters
    assert params[name].default is None and params["saxs_data"].default is None


# ------------------------------------------------------------------------------------------- the summaries of per-structure values
def _js_restated(metrics, values, ref_key, n_bins, weights, value_range):
    lo, hi = (values[ref_key].min(), values[ref_key].max()) if value_range is None else value_range
    hist = {k: np.histogram(v, bins=n_bins, weights=(weights or {}).get(k), range=(lo, hi))[0] + metrics.PSEUDO_C for k, v in values.items()}
    return {k: 0.0 if k == ref_key else np.around(metrics._js(h, hist[ref_key]), decimals=4) for k, h in hist.items()}


@pytest.mark.parametrize("value_range", (None, (0.0, 1.0)))
@pytest.mark.parametrize("weighted", (False, True))
def test_js_of_values_is_histogram_and_js(value_range, weighted):
    from str2str_amd.metrics import metrics

    rng = np.random.default_rng(11)
    values = {"target": rng.uniform(0.2, 0.8, size=9), "pred": rng.uniform(0.0, 1.0, size=7), "far": rng.uniform(100.0, 101.0, size=5)}
    weights = {"pred": rng.uniform(0.5, 2.0, size=7), "target": rng.uniform(0.5, 2.0, size=9)} if weighted else None
    for n_bins in (50, 12):
        got = metrics.js_of_values(values, "target", n_bins, weights, value_range)
        assert got == _js_restated(metrics, values, "target", n_bins, weights, value_range) and list(got) == ["pred", "far", "target"]
        lo, hi = value_range or (values["target"].min(), values["target"].max())
        ref_hist = np.histogram(values["target"], bins=n_bins, weights=(weights or {}).get("target"), range=(lo, hi))[0] + metrics.PSEUDO_C
        # nothing of ``far`` falls into the range: its histogram is the pseudo-count alone, a uniform distribution
        assert got["target"] == 0.0 and got["pred"] > 0.0 and got["far"] == np.around(metrics._js(np.ones(n_bins), ref_hist), decimals=4) > 0.0
    if value_range is not None:
        assert metrics.js_q_of(values, "target", 50, weights) == metrics.js_of_values(values, "target", 50, weights, (0.0, 1.0))
    assert metrics.js_of_values({"target": values["target"]}, "target", 50, None, value_range) == {"target": 0.0}
    with pytest.raises(ValueError, match="weights"):
        metrics.js_of_values(values, "target", 50, {"pred": np.ones(6)}, value_range)


def test_mean_of_values_is_numpy_average():
    from str2str_amd.metrics import metrics

    rng = np.random.default_rng(12)
    values = {"target": rng.normal(20.0, 3.0, size=9), "pred": rng.normal(25.0, 3.0, size=4)}
    w = {"pred": rng.uniform(0.5, 2.0, size=4)}
    assert metrics.mean_of_values(values) == {k: np.around(float(np.average(v)), decimals=4) for k, v in values.items()}
    assert metrics.mean_of_values(values) == {k: np.around(float(v.mean()), decimals=4) for k, v in values.items()}
    assert metrics.mean_of_values(values, w)["pred"] == np.around(float(np.average(values["pred"], weights=w["pred"])), decimals=4)
    assert metrics.mean_of_values(values, w)["target"] == metrics.mean_of_values(values)["target"]
    with pytest.raises(ValueError, match="weights"):
        metrics.mean_of_values(values, {"target": np.ones(4)})


def test_profiles_against_the_reference():
    from str2str_amd.metrics import metrics

    rng = np.random.default_rng(13)
    prop = {k: rng.dirichlet(np.ones(3), size=8) for k in ("target", "pred", "other")}
    got = metrics.against_reference(prop, "target")
    assert got == {"pred": np.around(np.abs(prop["pred"] - prop["target"]).mean(), decimals=4),
                   "other": np.around(np.abs(prop["other"] - prop["target"]).mean(), decimals=4), "target": 0.0}
    assert got["target"] == 0.0 and isinstance(got["target"], float) and got["pred"] > 0.0
    assert metrics.against_reference({"target": prop["target"], "pred": prop["target"].copy()})["pred"] == 0.0
    assert metrics.ss_mae_of(prop)["pred"] == np.around((0.5 * np.abs(prop["pred"] - prop["target"]).sum(1)).mean(), decimals=4)
    assert metrics.ss_mae_of(prop, "other")["other"] == 0.0
    helix, strand = metrics.ss_content_of(prop)
    assert helix == {k: np.around(p[:, 0].mean(), decimals=4) for k, p in prop.items()}
    assert strand == {k: np.around(p[:, 1].mean(), decimals=4) for k, p in prop.items()}
    curves = {k: rng.uniform(1.0, 50.0, size=6) for k in ("target", "pred")}
    assert metrics.saxs_mae_of(curves) == {"pred": np.around((np.abs(curves["pred"] - curves["target"]) / curves["target"]).mean(), decimals=4),
                                           "target": 0.0}
    maps = {k: (lambda m: (m + m.T) / 2.0)(rng.uniform(size=(9, 9))) for k in ("target", "pred")}
    upper = np.triu_indices(9, k=3)
    assert metrics.contact_mae_of(maps)["pred"] == np.around(np.abs(maps["pred"][upper] - maps["target"][upper]).mean(), decimals=4)
    assert metrics.contact_mae_of(maps, "target", 5)["pred"] == np.around(np.abs(maps["pred"] - maps["target"])[np.triu_indices(9, k=5)].mean(), decimals=4)
    assert metrics.contact_mae_of({k: m[:2, :2] for k, m in maps.items()}) == {"pred": 0.0, "target": 0.0}    # no pair 3 apart: empty profiles
    rows, w = rng.uniform(size=(5, 6)), rng.uniform(0.5, 2.0, size=5)
    assert (metrics.mean_curve(rows) == rows.mean(axis=0)).all() and (metrics.mean_curve(rows, w) == np.average(rows, axis=0, weights=w)).all()
    with pytest.raises(ValueError, match="weights"):
        metrics.mean_curve(rows, w[:-1])
    aatype = np.array([0, metrics.GLY, 14, metrics.GLY])
    exists = metrics._atom_exists(aatype)
    assert exists.dtype == np.uint8 and exists.tolist() == [[1] * 5, [1, 1, 1, 1, 0], [1] * 5, [1, 1, 1, 1, 0]]
    assert (metrics._host(torch.arange(3)) == np.arange(3)).all() and metrics._host([1, 2], np.float64).dtype == np.float64


# ------------------------------------------------------------------------------------------- the checks the wrappers share
def _wrapper_cases():
    ca, atoms = torch.zeros(2, 8, 3), torch.zeros(2, 8, 5, 3)
    seq = dict(aatype=np.zeros(8, dtype=int), residue_index=np.arange(8))
    exists = np.ones((8, 5), dtype=np.uint8)
    return {"backbone_violations": (dict(atoms=atoms, atom_exists=exists, **seq), "max_structures"),
            "secondary_structure": (dict(atoms=atoms, **seq), "max_structures"),
            "backbone_sasa": (dict(atoms=atoms, atom_exists=exists, radii=np.full((8, 5), 1.7)), "max_structures"),
            "ca_scattering": (dict(ca=ca, q=[0.0, 0.1]), "max_structures"),
            "ca_contact_map": (dict(ca=ca), "min_seq_sep"), "ca_contact_stats": (dict(ca=ca), "min_seq_sep"),
            "ca_native_contacts": (dict(native=torch.zeros(8, 3)), "min_seq_sep"),
            "ca_native_q": (dict(ca=ca, pairs=torch.zeros(5, 2, dtype=torch.int32), d0=torch.zeros(5, dtype=torch.float64)), None)}


@pytest.mark.parametrize("fn", list(_wrapper_cases()))
def test_wrappers_reject_bad_counts_before_the_device(fn, monkeypatch):
    from str2str_amd import ops
    from str2str_amd.ops import ensemble

    def touched(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(ensemble, "load_library", touched)
    kwargs, argument = _wrapper_cases()[fn]
    for bad in (0, -1, True, 1.5) if argument else ():
        with pytest.raises(ops.HipLibraryError, match="^" + re.escape(f"{fn}: {argument} must be an integer >= 1, got {bad}") + "$"):
            getattr(ops, fn)(**kwargs, **{argument: bad})
    with pytest.raises(ops.HipLibraryError, match="no CPU fallback"):
        getattr(ops, fn)(**kwargs)
