"""Entry point with the reference's CLI:  python eval.py task_name=inference [ckpt_path=…] [target_dir=null]
(reference: src/eval.py:102-173).  Composes configs/eval.yaml (hydra if installed, otherwise the built-in
composer), instantiates datamodule / model / trainer from their `_target_`s, loads the checkpoint with the
reference's key contract and runs ``trainer.predict``; when ``target_dir`` holds reference ensembles the samples are then
scored (src/eval.py:47-99) with the device metrics of str2str_amd/metrics (validity, bonding validity, JS-PwD, JS-TICA, JS-Rg;
``+extra_metrics=[...]`` adds columns out of EXTRA_METRICS, the backbone violations of the samples among them)
into the reference's tab-separated ``metrics_<tag>_<mmdd-HH-MM>.csv``.  ``+cluster_cutoff=<A>`` also clusters every sampled ensemble
(GROMOS at that RMSD, on the device) into ``clusters/<target>.pdb`` and ``clusters_<tag>_<mmdd-HH-MM>.csv`` next to it.
``+secondary_structure=true`` also assigns Kabsch & Sander's states to the sampled and the target ensembles (on the device) and writes
``ss_<tag>_<mmdd-HH-MM>.csv`` (helix and strand content, their distance from the target's, the Ramachandran JS distance) and the
per-residue propensities ``secondary_structure/<target>.csv``.
``+contacts=true`` also computes the CA contacts of the sampled and the target ensembles (on the device) and writes
``contacts_<tag>_<mmdd-HH-MM>.csv`` (mean fraction of native contacts Q of both, the JS distance of their Q distributions, the mean
absolute difference of their contact maps, mean relative contact order of both) and the contact probabilities ``contacts/<target>.csv``.
``+sasa=true`` also computes the solvent-accessible surface of the backbone and CB atoms of the sampled and the target ensembles (on the
device; no side chains) and writes ``sasa_<tag>_<mmdd-HH-MM>.csv`` (mean total surface of both, the JS distance of their distributions, the
mean absolute difference of their per-residue relative accessibilities) and the per-residue means ``sasa/<target>.csv``.
``+saxs=true`` also computes what a solution measurement would see of the sampled and the target ensembles (on the device: the Debye
scattering curve and the Kirkwood hydrodynamic radius of the CA beads; no hydration shell, no excluded volume, no form-factor table) and
writes ``saxs_<tag>_<mmdd-HH-MM>.csv`` (the mean relative difference of the two curves, the mean hydrodynamic radius of both, the JS
distance of their distributions) and the curves ``saxs/<target>.csv``; ``+saxs_data=DIR`` adds the reduced chi^2 of the sampled
ensemble's curve against the measured ``DIR/<target>.dat`` (columns q in 1/Angstrom, I, sigma).
``+dynamics=true`` also computes how the sampled and the target ensembles move (on the device: covariance of the superposed CA coordinates;
the eigenproblem on the host) and writes ``dynamics_<tag>_<mmdd-HH-MM>.csv`` (the JS distance of the projections on the target's first two
principal components, the RMSIP of the top ten, the mean absolute difference of the cross-correlation maps, the total variance of both)
and the cross-correlations ``dynamics/<target>.csv``.
``+tica_backend=device`` computes the ``js_tica`` column with the time-lagged covariances and the projections on the device
(metrics.js_tica(backend="device")); absent, the column is the reference's path.  Column name and file layout do not change.
``+msm=true`` (optional ``+msm_states=<k>``, default 100, and ``+msm_lag=<frames>``, default 20) also builds a Markov state model of the
target ensemble (TICA, k-means microstates and transition counts on the device; the estimators on the host) and writes
``msm_<tag>_<mmdd-HH-MM>.csv`` (the JS distance of the sampled ensemble's state populations from the target's, the number of active states,
the three slowest implied timescales of the target) and the per-state populations ``msm/<target>.csv``."""
import logging
import os
import sys
from functools import partial
from typing import Callable, NamedTuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("PROJECT_ROOT", ROOT)

from str2str_amd.metrics import metrics  # noqa: E402
from str2str_amd.utils import config as C  # noqa: E402

log = logging.getLogger("str2str_amd.eval")


def load_dotenv(path):
    if os.path.exists(path):
        for line in open(path):
            line = line.strip()
            if line and not line.startswith("#") and "=" in line:
                k, _, v = line.partition("=")
                os.environ.setdefault(k.strip(), v.strip().strip('"').strip("'"))


def load_model_checkpoint(model, ckpt_path):
    """.pth -> net weights only ('net.' prefix stripped, strict); .ckpt -> left to the trainer
    (reference src/utils/checkpoint_utils.py:3-27)."""
    if ckpt_path is None:
        return model, None
    if ckpt_path.endswith(".pth"):
        params = torch.load(ckpt_path, map_location=torch.device("cpu"))["state_dict"]
        model.net.load_state_dict({k.replace("net.", ""): v for k, v in params.items()})
        return model, None
    if ckpt_path.endswith(".ckpt"):
        return model, ckpt_path
    raise ValueError(f"ckpt_path {ckpt_path} is not a valid checkpoint file.")


# optional columns: the violations of the full backbone (peptide geometry, clashes); minimum RMSD under optimal superposition, TM-score under
# the identity correspondence, CA-lDDT (no superposition)
BACKBONE_METRICS = ("val_bb_bond", "val_bb_clash", "viol_per_residue")
EXTRA_METRICS = BACKBONE_METRICS + ("div_rmsd", "rmsd_recall", "rmsd_precision", "div_tm", "tm_recall", "tm_precision", "div_lddt", "lddt_recall", "lddt_precision")


def metric_columns(extra_metrics=None):
    """The reference's five columns in its order (src/eval.py:64-70), then the requested extra ones in the order asked for."""
    extra = [extra_metrics] if isinstance(extra_metrics, str) else list(extra_metrics or [])
    unknown = [m for m in extra if m not in EXTRA_METRICS]
    if unknown or len(set(extra)) != len(extra):
        raise ValueError(f"extra_metrics {extra}: expected distinct names out of {list(EXTRA_METRICS)}")
    return ["val_clash", "val_bond", "js_pwd", "js_rg", "js_tica"] + extra


CLUSTER_COLUMNS = ("n_clusters", "top1_population", "top5_population", "n_singletons")


def cluster_summary(sizes):
    """One row of the clusters csv from the non-increasing cluster sizes: populations are fractions of the ensemble."""
    sizes = np.asarray(sizes, dtype=np.int64)
    total = float(sizes.sum())
    return {"n_clusters": int(len(sizes)), "top1_population": np.around(sizes[:1].sum() / total, decimals=4),
            "top5_population": np.around(sizes[:5].sum() / total, decimals=4), "n_singletons": int((sizes == 1).sum())}


SS_COLUMNS = ("ss_helix", "ss_strand", "ss_helix_target", "ss_strand_target", "ss_mae", "js_rama")
SS_CLASSES = ("helix", "strand", "other")
CONTACT_COLUMNS = ("q_mean", "q_mean_target", "js_q", "contact_mae", "rco", "rco_target")
SASA_COLUMNS = ("sasa_mean", "sasa_mean_target", "js_sasa", "sasa_mae")
SAXS_COLUMNS = ("saxs_mae", "rh_mean", "rh_mean_target", "js_rh")
DYNAMICS_COLUMNS = ("js_pca", "rmsip", "dccm_mae", "var_total", "var_total_target")


def _switch(name, value) -> bool:
    """``+<name>=...`` as a bool: absent, null and false leave everything as it was."""
    if value is None or isinstance(value, bool):
        return bool(value)
    if isinstance(value, str) and value.strip().lower() in ("true", "false", "1", "0", "yes", "no"):
        return value.strip().lower() in ("true", "1", "yes")
    raise ValueError(f"{name} {value!r}: expected true or false")


def tica_backend_switch(value) -> str:
    """``+tica_backend=...`` as js_tica's backend: absent, null and "host" are the reference's path."""
    if value is None:
        return "host"
    if isinstance(value, str) and value.strip().lower() in ("host", "device"):
        return value.strip().lower()
    raise ValueError(f"tica_backend {value!r}: expected host or device")


MSM_COLUMNS = ("js_msm", "n_active", "timescale_1", "timescale_2", "timescale_3")
MSM_STATES, MSM_LAG = 100, 20
msm_switch = partial(_switch, "msm")


def msm_row(ca, n_states=MSM_STATES, lagtime=MSM_LAG):
    """-> (row {MSM_COLUMNS}, table {per state: the target's and the samples' populations and the target's stationary distribution, NaN
    outside the active set}).  Fewer target frames than the lag time (or than the states): warned about, the row stays NaN."""
    row, table = dict.fromkeys(MSM_COLUMNS, float("nan")), {}
    try:
        labels = metrics.msm_states(ca, ref_key="target", lagtime=lagtime, n_states=n_states)
    except ValueError as e:
        log.warning(f"msm: {e}")
        return row, table
    model = metrics.msm(labels["target"], n_states, lagtime)
    slowest = list(model.timescales[:3]) + [float("nan")] * 3
    row.update(js_msm=metrics.js_of_states(labels, n_states, "target")["pred"], n_active=int(len(model.active)),
               timescale_1=slowest[0], timescale_2=slowest[1], timescale_3=slowest[2])
    pi = np.full(n_states, np.nan)
    pi[model.active] = model.stationary
    table = {"state": np.arange(n_states), "population_target": metrics.state_populations(labels["target"], n_states),
             "population_pred": metrics.state_populations(labels["pred"], n_states), "stationary_target": pi}
    return row, table


def _backbones(what, pred_file, target_file):
    """-> ({"pred": atoms [R, L, 5, 3], "target": the same}, aatype, residue_index) of one target, the sequence being the samples'.  A
    target without a full backbone (a CA trace) is warned about and left out: its columns stay NaN."""
    from str2str_amd.common.pdb_utils import extract_backbone_atoms

    atoms, aatype, residue_index = extract_backbone_atoms(pred_file)
    both = {"pred": atoms}
    try:
        t_atoms = extract_backbone_atoms(target_file)[0]
        if t_atoms.shape[1] != atoms.shape[1]:
            raise ValueError(f"{t_atoms.shape[1]} residues for the samples' {atoms.shape[1]}")
        both["target"] = t_atoms
    except ValueError as e:
        log.warning(f"{what} of the target {target_file}: {e}")
    return both, aatype, residue_index


def _row(columns, values):
    """``columns`` filled with ``values`` from the left; NaN in those left over (the ones that need a target ensemble there is none of)."""
    return {**dict.fromkeys(columns, float("nan")), **dict(zip(columns, values))}


def _residue_table(residue_index, names, per_residue):
    """residue_index, then pred_<name> and target_<name> for every name out of {k: [len(names), L]}, rounded to 4 decimals (NaN for an
    ensemble that is not there)."""
    return {"residue_index": residue_index,
            **{f"{k}_{c}": np.around(per_residue[k][q], decimals=4) if k in per_residue else np.full(len(residue_index), np.nan)
               for k in ("pred", "target") for q, c in enumerate(names)}}


def secondary_structure_row(t):
    """One row of the ss csv and the per-residue propensities of both ensembles of the target ``t``."""
    both, aatype, residue_index = _backbones("secondary structure", t.pred_file, t.target_file)
    res = {k: metrics.secondary_structure_and_torsions(v, aatype, residue_index) for k, v in both.items()}   # the one launch per ensemble
    prop = {k: metrics._propensity(r[0].ss) for k, r in res.items()}
    helix, strand = metrics.ss_content_of(prop)
    values = (helix["pred"], strand["pred"])
    if "target" in both:
        js_rama = metrics.js_of_histograms({k: metrics._rama_histogram(*r[1:]) for k, r in res.items()})
        values += (helix["target"], strand["target"], metrics.ss_mae_of(prop)["pred"], js_rama["pred"])
    return _row(SS_COLUMNS, values), _residue_table(residue_index, SS_CLASSES, {k: p.T for k, p in prop.items()})


def contacts_row(t):
    """One row of the contacts csv and the table of contact probabilities (every pair i < j with either above 0) of both CA ensembles of
    the target ``t``.  The native of Q is the first structure of the target ensemble."""
    native = metrics.native_contacts(t.ca["target"][0])
    q = {k: metrics.q_of_contacts(v, *native) for k, v in t.ca.items()}
    p = {k: metrics.contact_map(v) for k, v in t.ca.items()}
    q_mean = metrics.mean_of_values(q)
    rco = metrics.mean_of_values({k: metrics.contact_order(v) for k, v in t.ca.items()})
    row = (q_mean["pred"], q_mean["target"], metrics.js_q_of(q)["pred"], metrics.contact_mae_of(p)["pred"], rco["pred"], rco["target"])
    i, j = np.nonzero(np.triu((p["pred"] > 0) | (p["target"] > 0)))
    return dict(zip(CONTACT_COLUMNS, row)), {"i": i, "j": j, "p_pred": np.around(p["pred"][i, j], decimals=4), "p_target": np.around(p["target"][i, j], decimals=4)}


def sasa_row(t):
    """One row of the sasa csv and the per-residue mean surface and mean relative accessibility of both ensembles of the target ``t``."""
    both, aatype, residue_index = _backbones("solvent accessibility", t.pred_file, t.target_file)
    res = {k: metrics.accessibility(v, aatype, residue_index) for k, v in both.items()}                      # the one launch on the chains per ensemble
    total, relative = {k: r[0].total for k, r in res.items()}, {k: r[1].mean(0) for k, r in res.items()}
    mean = metrics.mean_of_values(total)
    values = (mean["pred"],)
    if "target" in both:
        values += (mean["target"], metrics.js_of_values(total)["pred"], metrics.against_reference(relative)["pred"])
    return _row(SASA_COLUMNS, values), _residue_table(residue_index, ("sasa", "relative"), {k: (r[0].per_residue.mean(0), relative[k]) for k, r in res.items()})


def saxs_row(t):
    """One row of the saxs csv (with a directory of measured curves also ``saxs_chi2``: the reduced chi^2 of the sampled ensemble's curve
    on the measured file's own q grid, scaled to it by least squares; NaN where the file does not exist) and the curves of both CA
    ensembles of the target ``t`` on metrics.SAXS_Q_GRID."""
    res = {k: metrics.saxs_profile_and_rh(v, metrics.SAXS_Q_GRID) for k, v in t.ca.items()}                   # the one launch per ensemble
    curve, rh = {k: metrics.mean_curve(r[0]) for k, r in res.items()}, {k: r[1] for k, r in res.items()}
    rh_mean = metrics.mean_of_values(rh)
    row = dict(zip(SAXS_COLUMNS, (metrics.saxs_mae_of(curve)["pred"], rh_mean["pred"], rh_mean["target"], metrics.js_of_values(rh)["pred"])))
    if t.saxs_file is not None:
        row["saxs_chi2"] = float("nan")
        if os.path.isfile(t.saxs_file):
            q_exp, i_exp, sigma = metrics.read_saxs_dat(t.saxs_file)
            row["saxs_chi2"] = np.around(metrics.saxs_chi2(metrics.ensemble_saxs(t.ca["pred"], q_exp), i_exp, sigma)[0], decimals=4)
    return row, {"q": metrics.SAXS_Q_GRID, "i_pred": np.around(curve["pred"], decimals=4), "i_target": np.around(curve["target"], decimals=4)}


def dynamics_row(t):
    """One row of the dynamics csv and the cross-correlations (every pair i < j) of both CA ensembles of the target ``t``: the PCA of
    js_pca is the target ensemble's, the other columns live in the frame of its mean structure (metrics.dynamics_frame)."""
    try:
        covs = metrics.dynamics_frame(t.ca)                                                                   # the one superposition and covariance per ensemble
    except ValueError as e:                    # an ensemble of one structure does not move: the columns stay NaN, the table empty
        log.warning(f"dynamics of {t.pred_file}: {e}")
        return _row(DYNAMICS_COLUMNS, ()), dict.fromkeys(("i", "j", "c_pred", "c_target"), ())
    c = {k: metrics._dccm(v).cpu().numpy() for k, v in covs.items()}
    var = metrics.total_variance_of(covs)
    row = (metrics.js_pca(t.ca, return_pc=False)["pred"], metrics.rmsip_of(covs, {k: len(v) for k, v in t.ca.items()})["pred"],
           metrics.dccm_mae_of(c)["pred"], var["pred"], var["target"])
    i, j = np.triu_indices(len(c["pred"]), k=1)
    return dict(zip(DYNAMICS_COLUMNS, row)), {"i": i, "j": j, "c_pred": np.around(c["pred"][i, j], decimals=4), "c_target": np.around(c["target"][i, j], decimals=4)}


class Report(NamedTuple):
    """An optional report of ``evaluate_prediction``: ``+<name>=true`` switches it on, ``<name>/<target>.csv`` receives the table of every
    target and ``<prefix>_<tag>_<mmdd-HH-MM>.csv`` one row per target, with the mean row where ``mean_row`` says so."""
    name: str
    prefix: str
    columns: tuple
    row: Callable          # (the target: its files and CA ensembles) -> (row {column: value}, table {column: values})
    mean_row: bool


REPORTS = (Report("secondary_structure", "ss", SS_COLUMNS, secondary_structure_row, False), Report("contacts", "contacts", CONTACT_COLUMNS, contacts_row, True),
           Report("sasa", "sasa", SASA_COLUMNS, sasa_row, True), Report("saxs", "saxs", SAXS_COLUMNS, saxs_row, True),
           Report("dynamics", "dynamics", DYNAMICS_COLUMNS, dynamics_row, True))
secondary_structure_switch, contacts_switch, sasa_switch, saxs_switch, dynamics_switch = (partial(_switch, r.name) for r in REPORTS)


def _write_summary(output_dir, prefix, tag, rows, columns, mean_row):
    """``<prefix>_<tag>_<mmdd-HH-MM>.csv``: one row per target."""
    import pandas as pd
    from time import strftime

    frame = pd.DataFrame.from_dict(rows, orient="index", columns=list(columns))
    if mean_row:
        frame.loc["mean"] = np.around(frame.mean(), decimals=4)
    frame.to_csv(os.path.join(output_dir, f"{prefix}_{tag}_{strftime('%m%d-%H-%M')}.csv"), index=True, sep="\t")


def evaluate_prediction(pred_dir: str, target_dir: str = None, tag: str = None, extra_metrics=None, cluster_cutoff=None,
                        secondary_structure=None, contacts=None, sasa=None, saxs=None, saxs_data=None, dynamics=None, tica_backend=None,
                        msm=None, msm_states=None, msm_lag=None):
    """reference src/eval.py:47-99: one row per target, one column per metric, plus the mean row.  ``extra_metrics``: names out of
    EXTRA_METRICS, appended as columns after the reference's five (none by default: the file is then the reference's).
    ``cluster_cutoff`` (A; None: nothing of this happens): the ``pred`` ensemble of every target is clustered by ``metrics.cluster_rmsd``;
    ``clusters/<target>.pdb`` receives the centres' MODELs, most populated first, and ``clusters_<tag>_<mmdd-HH-MM>.csv`` one row per
    target (CLUSTER_COLUMNS), both next to the metrics csv.  ``secondary_structure``, ``contacts``, ``sasa``, ``saxs``, ``dynamics`` (true; otherwise
    nothing of it happens): the REPORTS on the ``pred`` and the ``target`` ensemble of every target.  Next to the metrics csv,
    ``ss_<tag>_<mmdd-HH-MM>.csv`` (SS_COLUMNS) and ``secondary_structure/<target>.csv`` receive the states' content and the per-residue
    propensities; ``contacts_...csv`` (CONTACT_COLUMNS) and ``contacts/<target>.csv`` the native-contact and contact-order summaries and
    the contact probabilities; ``sasa_...csv`` (SASA_COLUMNS) and ``sasa/<target>.csv`` the surface summaries and the per-residue mean
    surface and mean relative accessibility; ``saxs_...csv`` (SAXS_COLUMNS, and ``saxs_chi2`` against ``<saxs_data>/<target>.dat`` when
    the directory ``saxs_data`` is given) and ``saxs/<target>.csv`` the scattering summaries and the curves; ``dynamics_...csv``
    (DYNAMICS_COLUMNS) and ``dynamics/<target>.csv`` the essential-dynamics summaries and the cross-correlations.  All but the ss csv end
    with the mean row.  ``tica_backend`` ("device"; None or "host": the reference's path) selects how the ``js_tica`` column is computed.
    ``msm`` (true; otherwise nothing of it happens): ``msm_row`` on every target with ``msm_states`` microstates (default MSM_STATES) at the
    lag time ``msm_lag`` (default MSM_LAG); ``msm_...csv`` (MSM_COLUMNS, no mean row) and ``msm/<target>.csv`` receive the summaries and the
    per-state populations."""
    columns = metric_columns(extra_metrics)
    tica_backend = tica_backend_switch(tica_backend)
    switches = dict(secondary_structure=secondary_structure, contacts=contacts, sasa=sasa, saxs=saxs, dynamics=dynamics)
    reports = [r for r in REPORTS if _switch(r.name, switches[r.name])]
    if saxs_data is not None and not _switch("saxs", saxs):
        raise ValueError(f"saxs_data {saxs_data}: needs saxs=true")
    if cluster_cutoff is not None and not 0.0 < float(cluster_cutoff) < float("inf"):
        raise ValueError(f"cluster_cutoff {cluster_cutoff}: expected a positive finite RMSD in Angstrom")
    msm = msm_switch(msm)
    msm_size = {"msm_states": MSM_STATES, "msm_lag": MSM_LAG}
    for name, value in (("msm_states", msm_states), ("msm_lag", msm_lag)):
        if value is not None:
            if not msm:
                raise ValueError(f"{name} {value}: needs msm=true")
            if isinstance(value, bool) or not isinstance(value, int) or value < 1:
                raise ValueError(f"{name} {value!r}: expected an integer >= 1")
            msm_size[name] = value
    from time import strftime
    from types import SimpleNamespace

    import pandas as pd

    from str2str_amd.common.pdb_utils import extract_backbone_atoms, extract_backbone_coords, select_pdb_models

    if target_dir is None or not os.path.isdir(target_dir):
        log.warning(f"target_dir {target_dir} does not exist. Skip evaluation.")
        return {}
    assert os.path.isdir(pred_dir), f"pred_dir {pred_dir} is not a directory."
    targets = [d.replace(".pdb", "") for d in os.listdir(target_dir)]
    output_dir = os.path.dirname(os.path.dirname(os.path.abspath(pred_dir)))
    tag = tag if tag is not None else "dev"
    fns = {"val_clash": metrics.validity, "val_bond": metrics.bonding_validity, "js_pwd": metrics.js_pwd, "js_rg": metrics.js_rg,
           "js_tica": metrics.js_tica if tica_backend == "host" else partial(metrics.js_tica, backend=tica_backend),
           # (the reference's five columns, in its order: src/eval.py:64-70)
           "div_rmsd": metrics.diversity_rmsd, "div_tm": metrics.diversity_tm, "div_lddt": metrics.diversity_lddt}
    coverage = {"rmsd": metrics.coverage_rmsd, "tm": metrics.coverage_tm, "lddt": metrics.coverage_lddt}
    eval_res = {k: {} for k in columns}
    clusters, rows, msm_rows = {}, {r.name: {} for r in reports}, {}
    for target in targets:
        pred_file, target_file = os.path.join(pred_dir, f"{target}.pdb"), os.path.join(target_dir, f"{target}.pdb")
        if not os.path.isfile(pred_file):
            continue
        ca = {"target": extract_backbone_coords(target_file), "pred": extract_backbone_coords(pred_file)}
        shared = {}                            # what several columns read: computed once per target, when the first of them asks
        for name in columns:
            family, _, part = name.rpartition("_")
            try:
                if name in BACKBONE_METRICS:           # the violations of the sampled N, CA, C, O, CB
                    if "backbone" not in shared:
                        v = metrics.backbone_violations(*extract_backbone_atoms(pred_file))
                        shared["backbone"] = dict(zip(BACKBONE_METRICS, (*metrics.validity_of_violations(v), metrics.rate_of_violations(v))))
                    value = shared["backbone"][name]
                elif family in coverage:               # <family>_recall and <family>_precision
                    if family not in shared:
                        shared[family] = dict(zip(("recall", "precision"), coverage[family](ca, ref_key="target")))
                    value = shared[family][part]["pred"]
                else:
                    res = fns[name](ca, ref_key="target") if name.startswith("js_") else fns[name](ca)
                    value = res[0]["pred"] if name == "js_tica" else res["pred"]
            except (ValueError, NotImplementedError) as e:   # e.g. fewer reference frames than the TICA lag time: the other columns stand
                log.warning(f"{name} on {target}: {e}")
                value = float("nan")
            eval_res[name][target] = value
        if cluster_cutoff is not None:
            res = metrics.cluster_rmsd(ca["pred"], float(cluster_cutoff))
            select_pdb_models(pred_file, res.centres, os.path.join(output_dir, "clusters", f"{target}.pdb"))
            clusters[target] = cluster_summary(res.sizes)
        if msm:
            msm_rows[target], table = msm_row(ca, msm_size["msm_states"], msm_size["msm_lag"])
            os.makedirs(os.path.join(output_dir, "msm"), exist_ok=True)
            pd.DataFrame(table).to_csv(os.path.join(output_dir, "msm", f"{target}.csv"), index=False, sep="\t")
        files = SimpleNamespace(ca=ca, pred_file=pred_file, target_file=target_file,
                                saxs_file=None if saxs_data is None else os.path.join(str(saxs_data), f"{target}.dat"))
        for r in reports:
            rows[r.name][target], table = r.row(files)
            os.makedirs(os.path.join(output_dir, r.name), exist_ok=True)
            pd.DataFrame(table).to_csv(os.path.join(output_dir, r.name, f"{target}.csv"), index=False, sep="\t")
    df = pd.DataFrame.from_dict(eval_res)
    df.loc["mean"] = np.around(df.mean(), decimals=4)
    df.to_csv(os.path.join(output_dir, f"metrics_{tag}_{strftime('%m%d-%H-%M')}.csv"), index=True, sep="\t")
    if cluster_cutoff is not None:
        _write_summary(output_dir, "clusters", tag, clusters, CLUSTER_COLUMNS, False)
    if msm:
        _write_summary(output_dir, "msm", tag, msm_rows, MSM_COLUMNS, False)
    for r in reports:
        _write_summary(output_dir, r.prefix, tag, rows[r.name], r.columns + (("saxs_chi2",) if r.name == "saxs" and saxs_data is not None else ()), r.mean_row)
    return df.loc["mean"]


def evaluate(cfg):
    pred_dir = cfg.get("pred_dir")
    scoring = dict(target_dir=cfg.get("target_dir"), tag=cfg.get("task_name"), extra_metrics=cfg.get("extra_metrics"),
                   cluster_cutoff=cfg.get("cluster_cutoff"), secondary_structure=cfg.get("secondary_structure"),
                   contacts=cfg.get("contacts"), sasa=cfg.get("sasa"), saxs=cfg.get("saxs"), saxs_data=cfg.get("saxs_data"), dynamics=cfg.get("dynamics"),
                   tica_backend=cfg.get("tica_backend"), msm=cfg.get("msm"), msm_states=cfg.get("msm_states"), msm_lag=cfg.get("msm_lag"))
    if pred_dir and os.path.isdir(pred_dir):
        log.info(f"Found pre-computed prediction directory {pred_dir}.")
        return evaluate_prediction(pred_dir, **scoring)
    log.info(f"Instantiating datamodule <{cfg.data['_target_']}>")
    datamodule = C.instantiate(cfg.data)
    log.info(f"Instantiating model <{cfg.model['_target_']}>")
    model = C.instantiate(cfg.model)
    log.info(f"Instantiating trainer <{cfg.trainer['_target_']}>")
    trainer = C.instantiate(cfg.trainer)
    if cfg.get("ckpt_path"):
        model, ckpt_path = load_model_checkpoint(model, cfg.ckpt_path)
    else:
        from str2str_amd.synth import synth_state_dict

        log.warning("ckpt_path is null: using seeded synthetic weights (smoke run, not a trained model)")
        man = [(k, tuple(v.shape)) for k, v in model.net.state_dict().items()]
        model.net.load_state_dict(synth_state_dict(man, seed=0, sigma_final=0.002))
        ckpt_path = None
    datamodule.setup(stage="predict")
    dataloaders = datamodule.test_dataloader()
    if cfg.get("dry_run"):
        log.info(f"dry_run: {len(dataloaders)} target(s) featurised, model + checkpoint ready; not sampling.")
        return None
    if cfg.get("seed") is not None:   # (an extra key of this build: `seed=7` fixes the host noise stream; every rank seeds alike --
        torch.manual_seed(int(cfg.get("seed")))   #  the ranks then draw each chunk's noise identically and slice it, see sampler.py)
    log.info("Starting predictions.")
    pred_dir = trainer.predict(model=model, dataloaders=dataloaders, ckpt_path=ckpt_path)[-1]
    log.info(f"Samples written under {pred_dir}.")
    if int(os.environ.get("RANK", "0")) == 0 and cfg.get("target_dir"):
        log.info(f"metrics: {dict(evaluate_prediction(pred_dir, **scoring))}")
    return pred_dir


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s][%(name)s][%(levelname)s] - %(message)s")
    load_dotenv(os.path.join(ROOT, ".env"))
    args = list(sys.argv[1:] if argv is None else argv)
    cfg = C.compose(os.path.join(ROOT, "configs"), "eval.yaml", args)
    # `trainer.devices=N` / `trainer=ddp` from a bare shell: start N ranks, one per GPU, as Lightning does behind the reference's
    # trainer.predict (src/eval.py:129,154; configs/trainer/ddp.yaml).  Inside a torch.distributed.run job this is one of the ranks.
    from str2str_amd.utils.launch import in_distributed_job, relaunch, resolve_devices

    n_dev = resolve_devices(cfg.trainer.get("devices", 1)) if cfg.trainer.get("accelerator", "gpu") != "cpu" else 1
    if n_dev > 1 and not in_distributed_job() and not cfg.get("dry_run") and not (cfg.get("pred_dir") and os.path.isdir(cfg.get("pred_dir"))):
        rc = relaunch(n_dev, __file__, args)
        if argv is None:
            sys.exit(rc)
        if rc:
            raise RuntimeError(f"eval.py: the {n_dev}-rank job exited with code {rc}")
        return None
    if cfg.get("extras", {}).get("print_config") and int(os.environ.get("RANK", "0")) == 0:
        import yaml

        log.info("config:\n" + yaml.safe_dump(C.to_plain(cfg), sort_keys=False, default_flow_style=False))
    return evaluate(cfg)


if __name__ == "__main__":
    main()
