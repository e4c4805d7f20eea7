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
ensemble's curve against the measured ``DIR/<target>.dat`` (columns q in 1/Angstrom, I, sigma)."""
import logging
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("PROJECT_ROOT", ROOT)

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
    import numpy as np

    sizes = np.asarray(sizes, dtype=np.int64)
    total = float(sizes.sum())
    return {"n_clusters": int(len(sizes)), "top1_population": np.around(sizes[:1].sum() / total, decimals=4),
            "top5_population": np.around(sizes[:5].sum() / total, decimals=4), "n_singletons": int((sizes == 1).sum())}


SS_COLUMNS = ("ss_helix", "ss_strand", "ss_helix_target", "ss_strand_target", "ss_mae", "js_rama")
SS_CLASSES = ("helix", "strand", "other")


def _switch(name, value) -> bool:
    if value is None or isinstance(value, bool):
        return bool(value)
    if isinstance(value, str) and value.strip().lower() in ("true", "false", "1", "0", "yes", "no"):
        return value.strip().lower() in ("true", "1", "yes")
    raise ValueError(f"{name} {value!r}: expected true or false")


def secondary_structure_switch(value) -> bool:
    """``+secondary_structure=...`` as a bool: absent, null and false leave everything as it was."""
    return _switch("secondary_structure", value)


CONTACT_COLUMNS = ("q_mean", "q_mean_target", "js_q", "contact_mae", "rco", "rco_target")


def contacts_switch(value) -> bool:
    """``+contacts=...`` as a bool: absent, null and false leave everything as it was."""
    return _switch("contacts", value)


def contacts_row(ca):
    """One row of the contacts csv (CONTACT_COLUMNS) and the table of contact probabilities (i, j, p_pred, p_target: every pair i < j with
    either above 0) of one target from its CA ensembles {"pred": [R, L, 3], "target": [Rt, L, 3]}.  The native of Q is the first structure
    of the target ensemble."""
    import numpy as np

    from str2str_amd.metrics import metrics

    q = metrics.mean_q(ca, ref_key="target")
    rco = {k: np.around(float(metrics.contact_order(v).mean()), decimals=4) for k, v in ca.items()}
    row = {"q_mean": q["pred"], "q_mean_target": q["target"], "js_q": metrics.js_q(ca, ref_key="target")["pred"],
           "contact_mae": metrics.contact_mae(ca, ref_key="target")["pred"], "rco": rco["pred"], "rco_target": rco["target"]}
    p = {k: metrics.contact_map(v) for k, v in ca.items()}
    i, j = np.nonzero(np.triu((p["pred"] > 0) | (p["target"] > 0)))
    return row, {"i": i, "j": j, "p_pred": np.around(p["pred"][i, j], decimals=4), "p_target": np.around(p["target"][i, j], decimals=4)}


SASA_COLUMNS = ("sasa_mean", "sasa_mean_target", "js_sasa", "sasa_mae")


def sasa_switch(value) -> bool:
    """``+sasa=...`` as a bool: absent, null and false leave everything as it was."""
    return _switch("sasa", value)


def sasa_row(pred_file, target_file, log=log):
    """One row of the sasa csv (SASA_COLUMNS) and the per-residue means {"pred": (sasa [L], relative [L]), "target": the same or None} of
    one target.  A target without a full backbone (a CA trace) leaves NaN in the columns that need it."""
    import numpy as np

    from str2str_amd.common.pdb_utils import extract_backbone_atoms
    from str2str_amd.metrics import metrics

    atoms, aatype, residue_index = extract_backbone_atoms(pred_file)
    both = {"pred": atoms}
    try:
        t_atoms, _, _ = extract_backbone_atoms(target_file)
        if t_atoms.shape[1] != atoms.shape[1]:
            raise ValueError(f"{t_atoms.shape[1]} residues for the samples' {atoms.shape[1]}")
        both["target"] = t_atoms
    except ValueError as e:
        log.warning(f"solvent accessibility of the target {target_file}: {e}")
    row = dict.fromkeys(SASA_COLUMNS, float("nan"))
    per_res = {k: (metrics.solvent_accessibility(v, aatype, residue_index).per_residue.mean(0),
                   metrics.relative_accessibility(v, aatype, residue_index).mean(0)) for k, v in both.items()}
    mean = metrics.mean_sasa(both, aatype, residue_index)
    row["sasa_mean"] = mean["pred"]
    if "target" in both:
        row["sasa_mean_target"] = mean["target"]
        row["js_sasa"] = metrics.js_sasa(both, ref_key="target", aatype=aatype, residue_index=residue_index)["pred"]
        row["sasa_mae"] = np.around(float(np.abs(per_res["pred"][1] - per_res["target"][1]).mean()), decimals=4)
    return row, {"pred": per_res["pred"], "target": per_res.get("target")}, residue_index


SAXS_COLUMNS = ("saxs_mae", "rh_mean", "rh_mean_target", "js_rh")


def saxs_switch(value) -> bool:
    """``+saxs=...`` as a bool: absent, null and false leave everything as it was."""
    return _switch("saxs", value)


def saxs_row(ca, data_file=None):
    """One row of the saxs csv (SAXS_COLUMNS; with ``data_file``, a path, also ``saxs_chi2``) and the table of the curves (q, i_pred,
    i_target on metrics.SAXS_Q_GRID) of one target from its CA ensembles {"pred": [R, L, 3], "target": [Rt, L, 3]}.  ``saxs_chi2`` is the
    reduced chi^2 of the sampled ensemble's curve, on the measured file's own q grid and scaled to it by least squares, and NaN where the
    file does not exist."""
    import numpy as np

    from str2str_amd.metrics import metrics

    q = metrics.SAXS_Q_GRID
    curve = {k: metrics.ensemble_saxs(v, q) for k, v in ca.items()}
    rh = metrics.mean_rh(ca)
    row = {"saxs_mae": np.around(float((np.abs(curve["pred"] - curve["target"]) / curve["target"]).mean()), decimals=4),
           "rh_mean": rh["pred"], "rh_mean_target": rh["target"], "js_rh": metrics.js_rh(ca, ref_key="target")["pred"]}
    if data_file is not None:
        row["saxs_chi2"] = float("nan")
        if os.path.isfile(data_file):
            q_exp, i_exp, sigma = metrics.read_saxs_dat(data_file)
            row["saxs_chi2"] = np.around(metrics.saxs_chi2(metrics.ensemble_saxs(ca["pred"], q_exp), i_exp, sigma)[0], decimals=4)
    return row, {"q": q, "i_pred": np.around(curve["pred"], decimals=4), "i_target": np.around(curve["target"], decimals=4)}


def secondary_structure_row(pred_file, target_file, log=log):
    """One row of the ss csv (SS_COLUMNS) and the per-residue propensities {"pred": [L, 3], "target": [L, 3] or None} of one target.  A
    target without a full backbone (a CA trace) leaves NaN in the columns that need it."""
    import numpy as np

    from str2str_amd.common.pdb_utils import extract_backbone_atoms
    from str2str_amd.metrics import metrics

    atoms, aatype, residue_index = extract_backbone_atoms(pred_file)
    both = {"pred": atoms}
    try:
        t_atoms, t_aatype, t_index = extract_backbone_atoms(target_file)
        if t_atoms.shape[1] != atoms.shape[1]:
            raise ValueError(f"{t_atoms.shape[1]} residues for the samples' {atoms.shape[1]}")
        both["target"] = t_atoms
    except ValueError as e:
        log.warning(f"secondary structure of the target {target_file}: {e}")
    row = dict.fromkeys(SS_COLUMNS, float("nan"))
    prop = metrics.ss_propensity(both, aatype, residue_index)
    row["ss_helix"], row["ss_strand"] = (np.around(float(prop["pred"][:, q].mean()), decimals=4) for q in (0, 1))
    if "target" in both:
        row["ss_helix_target"], row["ss_strand_target"] = (np.around(float(prop["target"][:, q].mean()), decimals=4) for q in (0, 1))
        row["ss_mae"] = np.around(float((0.5 * np.abs(prop["pred"] - prop["target"]).sum(1)).mean()), decimals=4)
        row["js_rama"] = metrics.js_rama(both, ref_key="target", residue_index=residue_index)["pred"]
    return row, {"pred": prop["pred"], "target": prop.get("target")}, residue_index


def evaluate_prediction(pred_dir: str, target_dir: str = None, tag: str = None, extra_metrics=None, cluster_cutoff=None,
                        secondary_structure=None, contacts=None, sasa=None, saxs=None, saxs_data=None):
    """reference src/eval.py:47-99: one row per target, one column per metric, plus the mean row.  ``extra_metrics``: names out of
    EXTRA_METRICS, appended as columns after the reference's five (none by default: the file is then the reference's).
    ``cluster_cutoff`` (A; None: nothing of this happens): the ``pred`` ensemble of every target is clustered by ``metrics.cluster_rmsd``;
    ``clusters/<target>.pdb`` receives the centres' MODELs, most populated first, and ``clusters_<tag>_<mmdd-HH-MM>.csv`` one row per
    target (CLUSTER_COLUMNS), both next to the metrics csv.  ``secondary_structure`` (true; otherwise nothing of this happens): the
    states of the ``pred`` and the ``target`` ensemble of every target; ``ss_<tag>_<mmdd-HH-MM>.csv`` receives one row per target
    (SS_COLUMNS) and ``secondary_structure/<target>.csv`` the per-residue propensities of both.  ``contacts`` (true; otherwise nothing of
    this happens): ``contacts_<tag>_<mmdd-HH-MM>.csv`` receives one row per target (CONTACT_COLUMNS) and the mean row, and
    ``contacts/<target>.csv`` the contact probabilities of both ensembles.  ``sasa`` (true; otherwise nothing of this happens):
    ``sasa_<tag>_<mmdd-HH-MM>.csv`` receives one row per target (SASA_COLUMNS) and the mean row, and ``sasa/<target>.csv`` the per-residue
    mean surface and mean relative accessibility of both ensembles.  ``saxs`` (true; otherwise nothing of this happens):
    ``saxs_<tag>_<mmdd-HH-MM>.csv`` receives one row per target (SAXS_COLUMNS, and ``saxs_chi2`` against ``<saxs_data>/<target>.dat`` when
    the directory ``saxs_data`` is given) and the mean row, and ``saxs/<target>.csv`` the scattering curves of both ensembles."""
    columns = metric_columns(extra_metrics)
    secondary_structure = secondary_structure_switch(secondary_structure)
    contacts = contacts_switch(contacts)
    sasa = sasa_switch(sasa)
    saxs = saxs_switch(saxs)
    if saxs_data is not None and not saxs:
        raise ValueError(f"saxs_data {saxs_data}: needs saxs=true")
    if cluster_cutoff is not None and not 0.0 < float(cluster_cutoff) < float("inf"):
        raise ValueError(f"cluster_cutoff {cluster_cutoff}: expected a positive finite RMSD in Angstrom")
    from time import strftime

    import numpy as np
    import pandas as pd

    from str2str_amd.common.pdb_utils import extract_backbone_atoms, extract_backbone_coords, select_pdb_models
    from str2str_amd.metrics import metrics

    if target_dir is None or not os.path.isdir(target_dir):
        log.warning(f"target_dir {target_dir} does not exist. Skip evaluation.")
        return {}
    assert os.path.isdir(pred_dir), f"pred_dir {pred_dir} is not a directory."
    targets = [d.replace(".pdb", "") for d in os.listdir(target_dir)]
    output_dir = os.path.dirname(os.path.dirname(os.path.abspath(pred_dir)))
    tag = tag if tag is not None else "dev"
    fns = {"val_clash": metrics.validity, "val_bond": metrics.bonding_validity, "js_pwd": metrics.js_pwd, "js_rg": metrics.js_rg,
           "js_tica": metrics.js_tica,   # the reference's five columns, in its order (src/eval.py:64-70)
           "div_rmsd": metrics.diversity_rmsd, "div_tm": metrics.diversity_tm, "div_lddt": metrics.diversity_lddt}
    coverage = {"rmsd": metrics.coverage_rmsd, "tm": metrics.coverage_tm, "lddt": metrics.coverage_lddt}
    eval_res = {k: {} for k in columns}
    clusters, ss_rows, contact_rows, sasa_rows, saxs_rows = {}, {}, {}, {}, {}
    for target in targets:
        pred_file = os.path.join(pred_dir, f"{target}.pdb")
        if not os.path.isfile(pred_file):
            continue
        ca = {"target": extract_backbone_coords(os.path.join(target_dir, f"{target}.pdb")), "pred": extract_backbone_coords(pred_file)}
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
        if secondary_structure:
            ss_rows[target], prop, numbers = secondary_structure_row(pred_file, os.path.join(target_dir, f"{target}.pdb"))
            table = {"residue_index": numbers}
            for k in ("pred", "target"):
                for q, c in enumerate(SS_CLASSES):
                    table[f"{k}_{c}"] = np.full(len(numbers), np.nan) if prop[k] is None else np.around(prop[k][:, q], decimals=4)
            os.makedirs(os.path.join(output_dir, "secondary_structure"), exist_ok=True)
            pd.DataFrame(table).to_csv(os.path.join(output_dir, "secondary_structure", f"{target}.csv"), index=False, sep="\t")
        if contacts:
            contact_rows[target], table = contacts_row(ca)
            os.makedirs(os.path.join(output_dir, "contacts"), exist_ok=True)
            pd.DataFrame(table).to_csv(os.path.join(output_dir, "contacts", f"{target}.csv"), index=False, sep="\t")
        if sasa:
            sasa_rows[target], per_res, numbers = sasa_row(pred_file, os.path.join(target_dir, f"{target}.pdb"))
            table = {"residue_index": numbers}
            for k in ("pred", "target"):
                for q, c in enumerate(("sasa", "relative")):
                    table[f"{k}_{c}"] = np.full(len(numbers), np.nan) if per_res[k] is None else np.around(per_res[k][q], decimals=4)
            os.makedirs(os.path.join(output_dir, "sasa"), exist_ok=True)
            pd.DataFrame(table).to_csv(os.path.join(output_dir, "sasa", f"{target}.csv"), index=False, sep="\t")
        if saxs:
            saxs_rows[target], table = saxs_row(ca, None if saxs_data is None else os.path.join(str(saxs_data), f"{target}.dat"))
            os.makedirs(os.path.join(output_dir, "saxs"), exist_ok=True)
            pd.DataFrame(table).to_csv(os.path.join(output_dir, "saxs", f"{target}.csv"), index=False, sep="\t")
    df = pd.DataFrame.from_dict(eval_res)
    df.loc["mean"] = np.around(df.mean(), decimals=4)
    df.to_csv(os.path.join(output_dir, f"metrics_{tag}_{strftime('%m%d-%H-%M')}.csv"), index=True, sep="\t")
    if cluster_cutoff is not None:
        pd.DataFrame.from_dict(clusters, orient="index", columns=list(CLUSTER_COLUMNS)).to_csv(
            os.path.join(output_dir, f"clusters_{tag}_{strftime('%m%d-%H-%M')}.csv"), index=True, sep="\t")
    if secondary_structure:
        pd.DataFrame.from_dict(ss_rows, orient="index", columns=list(SS_COLUMNS)).to_csv(
            os.path.join(output_dir, f"ss_{tag}_{strftime('%m%d-%H-%M')}.csv"), index=True, sep="\t")
    if contacts:
        cf = pd.DataFrame.from_dict(contact_rows, orient="index", columns=list(CONTACT_COLUMNS))
        cf.loc["mean"] = np.around(cf.mean(), decimals=4)
        cf.to_csv(os.path.join(output_dir, f"contacts_{tag}_{strftime('%m%d-%H-%M')}.csv"), index=True, sep="\t")
    if sasa:
        sf = pd.DataFrame.from_dict(sasa_rows, orient="index", columns=list(SASA_COLUMNS))
        sf.loc["mean"] = np.around(sf.mean(), decimals=4)
        sf.to_csv(os.path.join(output_dir, f"sasa_{tag}_{strftime('%m%d-%H-%M')}.csv"), index=True, sep="\t")
    if saxs:
        xf = pd.DataFrame.from_dict(saxs_rows, orient="index", columns=list(SAXS_COLUMNS) + ([] if saxs_data is None else ["saxs_chi2"]))
        xf.loc["mean"] = np.around(xf.mean(), decimals=4)
        xf.to_csv(os.path.join(output_dir, f"saxs_{tag}_{strftime('%m%d-%H-%M')}.csv"), index=True, sep="\t")
    return df.loc["mean"]


def evaluate(cfg):
    pred_dir = cfg.get("pred_dir")
    scoring = dict(target_dir=cfg.get("target_dir"), tag=cfg.get("task_name"), extra_metrics=cfg.get("extra_metrics"),
                   cluster_cutoff=cfg.get("cluster_cutoff"), secondary_structure=cfg.get("secondary_structure"),
                   contacts=cfg.get("contacts"), sasa=cfg.get("sasa"), saxs=cfg.get("saxs"), saxs_data=cfg.get("saxs_data"))
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
