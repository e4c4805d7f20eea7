"""Solution scattering without a GPU: the yardstick (tests/ref_saxs.py) held to closed forms it did not produce, the C-ABI surface, the
argument checks, the numpy tails of the ensemble metrics, the fit against a measured curve, the reader of measured curves and the
evaluation switch."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import ref_saxs as ref
import saxs_cases as cases
from conftest import ROOT

ULP = 2.0 ** -52


def _beads(*points):
    return np.asarray(points, dtype=np.float32)[None]


# ------------------------------------------------------------------------------------------------------------------ closed forms
def test_one_bead():
    q = np.array([0.0, 0.1, 0.6])
    table = np.array([[1.0, 1.0, 1.0], [-2.5, 0.5, 3.0]])
    intensity, inv = ref.scattering(_beads((3.0, -2.0, 7.5)), q, [1], table)
    assert intensity.tolist() == [[6.25, 0.25, 9.0]] and inv.tolist() == [0.0]
    assert ref.scattering(_beads((3.0, -2.0, 7.5)), q)[0].tolist() == [[1.0, 1.0, 1.0]]
    assert ref.hydrodynamic_radius(_beads((3.0, -2.0, 7.5))).tolist() == [np.inf]


def test_dumbbell():
    d, f1, f2 = 4.0, 1.5, -0.75
    q = np.array([0.0, 0.05, 0.3, 0.6, math.pi / d])
    table = np.stack([np.full(len(q), f1), np.full(len(q), f2)])
    x = _beads((1.0, 2.0, -1.0), (1.0, 2.0 + d, -1.0))
    intensity, inv = ref.scattering(x, q, [0, 1], table)
    a = q * d
    want = f1 * f1 + f2 * f2 + 2.0 * f1 * f2 * np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    assert (np.abs(intensity[0] - want) <= 4 * ULP * (abs(f1) + abs(f2)) ** 2).all()
    assert intensity[0, 0] == (f1 + f2) ** 2
    cross = abs(intensity[0, -1] - (f1 * f1 + f2 * f2))          # q d = pi: the cross term vanishes but for the rounding of pi
    print(f"dumbbell at q = pi / d: cross term {cross:.3e}")
    assert cross <= 2.0 ** -50 * abs(2.0 * f1 * f2)
    assert inv[0] == 1.0 / (2.0 * d) and ref.hydrodynamic_radius(x)[0] == 2.0 * d


def test_regular_tetrahedron():
    x = _beads((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)) * np.float32(1.5)
    d = 1.5 * math.sqrt(8.0)
    q = np.array([0.0, 0.07, 0.3, 0.6])
    intensity, inv = ref.scattering(x, q)
    a = q * d
    want = 4.0 + 12.0 * np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    assert (np.abs(intensity[0] - want) <= 8 * ULP * 16.0).all() and intensity[0, 0] == 16.0
    rh = ref.hydrodynamic_radius(x)[0]                          # L^2 / (12 / d) = 4 d / 3
    assert abs(rh - 4.0 * d / 3.0) <= 4 * ULP * rh
    coincident = _beads((1, 1, 1), (2, 0, 0), (1, 1, 1))
    intensity, inv = ref.scattering(coincident, [0.3])
    assert inv[0] == np.inf and ref.hydrodynamic_radius(coincident)[0] == 0.0
    a = 0.3 * math.sqrt(3.0)
    assert abs(intensity[0, 0] - (3.0 + 2.0 * (1.0 + 2.0 * math.sin(a) / a))) <= 8 * ULP * 9.0     # s = 1 for the coincident pair


@pytest.mark.parametrize("tag", ("L13_R17_T3", "L31_R9_T21", "L65_R17_T3"))
def test_forward_scattering_is_the_squared_sum_of_signed_form_factors(tag):
    c = cases.case(tag)
    q = np.zeros(len(c.q))
    got = ref.scattering(c.ca, q, c.types, c.table)[0]
    f = c.table[c.types]
    L = c.ca.shape[1]
    assert (f < 0).any() and (f > 0).any()
    bound = (L * (L + 1) // 2 + 16) * ULP * np.abs(f).sum(0) ** 2
    assert (np.abs(got - f.sum(0)[None] ** 2) <= bound[None]).all()
    assert (ref.scattering(c.ca, q)[0] == float(L * L)).all()  # the default form factors: I(0) = L^2, exactly (integers)


def test_scaling_by_a_power_of_two_is_exact():
    c = cases.case("L31_R9")
    q = cases.q_list(17)
    for s in (2.0, 0.25):
        a = ref.scattering(c.ca * np.float32(s), q)
        b = ref.scattering(c.ca, q * s)
        assert a[0].tobytes() == b[0].tobytes() and (a[1] * s).tobytes() == b[1].tobytes()


@pytest.mark.parametrize("tag", ("L13_R17", "L65_R17"))
def test_rigid_motion(tag):
    """A rigid motion that float32 represents exactly: coordinates on a grid of 2^-10 A, a cyclic permutation of the axes with two signs
    flipped (a proper rotation) and a shift on the grid.  Every difference is then the same number, only the order of the three squares
    in a sum changes: within the device test's bound, (N + 16) 2^-52 L^2."""
    c = cases.case(tag)
    x = (np.round(c.ca.astype(np.float64) * 1024.0) / 1024.0).astype(np.float32)
    moved = (np.stack([-x[..., 1], x[..., 2], -x[..., 0]], axis=-1) + np.array([37.0, -12.5, 3.0 + 1.0 / 1024.0])).astype(np.float32)
    assert ((moved.astype(np.float64) - np.array([37.0, -12.5, 3.0 + 1.0 / 1024.0]))[..., 0] == -x[..., 1].astype(np.float64)).all()
    L = x.shape[1]
    a, b = ref.scattering(x, c.q), ref.scattering(moved, c.q)
    bound = (L * (L + 1) // 2 + 16) * ULP
    print(f"{tag}: rigid motion moves I by {np.abs(a[0] - b[0]).max() / (bound * L * L):.2e} of the bound")
    assert (np.abs(a[0] - b[0]) <= bound * L * L).all() and (np.abs(a[1] - b[1]) <= bound * a[1]).all()
    assert not np.array_equal(x, moved)


@pytest.mark.parametrize("L,R", ((13, 17), (65, 17), (257, 2)))
def test_guinier_identity(L, R):
    """0 <= Rg^2 - (3 / q^2)(1 - I(q) / L^2) <= (q r_max)^2 Rg^2 / 20, from 0 <= s(a) - (1 - a^2 / 6) <= a^4 / 120 and mean r^2 = 2 Rg^2."""
    ca, _ = cases.ca_ensemble(L, R)
    q = 1e-3
    intensity = ref.scattering(ca, [q])[0][:, 0]
    rg2 = ref.radius_of_gyration_sq(ca)
    r_max = ref.pair_distances(ca.astype(np.float64))[0].max(axis=1)
    gap = rg2 - (3.0 / (q * q)) * (1.0 - intensity / float(L * L))
    print(f"L = {L}: Guinier gap {gap.min() / rg2.max():.2e} .. {(gap / rg2).max():.2e} of Rg^2")
    assert (gap >= 0.0).all() and (gap <= (q * r_max) ** 2 * rg2 / 20.0).all()


def test_nan_stays_in_its_structure():
    c = cases.case("L13_R17")
    clean = ref.scattering(c.ca, c.q)
    x = c.ca.copy()
    x[5, 7, 1] = np.nan
    dirty = ref.scattering(x, c.q)
    keep = np.arange(17) != 5
    assert np.isnan(dirty[0][5]).all() and np.isnan(dirty[1][5])
    assert dirty[0][keep].tobytes() == clean[0][keep].tobytes() and dirty[1][keep].tobytes() == clean[1][keep].tobytes()
    one = ref.scattering(_beads((np.nan, 0.0, 0.0)), [0.0, 0.1])
    assert np.isnan(one[0]).all() and np.isnan(one[1]).all()   # a structure of one bead has no pair to carry the NaN


def test_the_cases_cover_what_they_are_there_for():
    assert set(cases.SHAPES) == {(1, 2), (2, 1), (3, 4), (13, 17), (23, 3), (24, 3), (31, 9), (64, 3), (65, 17), (257, 2)}
    assert 23 * 22 // 2 == 253 < 256 < 276 == 24 * 23 // 2 and cases.LONG == (1024, 1) and len(cases.LONG_Q) == 3
    assert cases.N_Q == (1, 15, 16, 17, 33) and cases.MANY_Q == (13, 2, 1024) and cases.N_TYPES == (1, 3, 21)
    q = np.asarray(cases.Q_DEFAULT)
    assert q.min() == 0.0 and q.max() == 0.6 and len(set(q.tolist())) < len(q)
    for n in (17, 33, 1024):
        q = cases.q_list(n)
        assert len(q) == n and q.min() == 0.0 and q.max() == 0.6 and len(set(q.tolist())) == n - 1
    for n in cases.N_TYPES:
        c = cases.case(f"L31_R9_T{n}")
        assert c.table.shape == (n, len(c.q)) and (c.table[:, 1] < 0).all() and set(c.types.tolist()) == set(range(n)) and c.types.dtype == np.int32
        assert n < 3 or ((c.table[1, [0, 2]] < 0).all() and (c.table[0, [0, 2]] > 0).all())
    assert len(cases.tags()) == len(set(cases.tags())) == 10 + 1 + 5 + 1 + 6


# ------------------------------------------------------------------------------------------------------------ header and binding
def test_abi_and_interface_are_declared():
    from str2str_amd import build, ops
    from str2str_amd.metrics import metrics
    from str2str_amd.ops import binding, ensemble

    text = open(os.path.join(ROOT, "include", "str2str_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"^int\s+(s2s_\w+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M))
    name = "s2s_ca_scattering"
    assert name in protos and name in ops.EXPORTS
    args = [" ".join(a.split()) for a in protos[name].split(",")]
    assert args == ["const float* ca", "int n", "int n_res", "const double* q", "int n_q", "const int* types", "const double* table", "int n_types",
                    "double* intensity", "double* inv_r_mean", "void* stream"]
    assert len(args) == len(binding._SIGNATURES[name]) == 11
    for macro, value in (("S2S_SAXS_MAX_RES", ops.SAXS_MAX_RES), ("S2S_SAXS_MAX_Q", ops.SAXS_MAX_Q), ("S2S_SAXS_MAX_TYPES", ops.SAXS_MAX_TYPES)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", hdr).group(1)) == value == getattr(ensemble, macro[4:])
    assert (ops.SAXS_MAX_RES, ops.SAXS_MAX_Q, ops.SAXS_MAX_TYPES) == (1024, 1024, 64)
    assert ops.ABI_VERSION == 40
    assert int(re.search(r"return (\d+);", open(os.path.join(ROOT, "str2str_amd", "csrc", "abi.hip")).read()).group(1)) == 40
    assert build.UNITS["ensemble_saxs.hip"] == ["-ffp-contract=off"]
    section = text.split("Solution scattering")[1].split("S2S_SAXS_MAX_RES")[0]
    for said in ("Debye", "Kirkwood", "no hydration shell", "no excluded-volume term", "no built-in residue form-factor table", "no side chains",
                 "Nygaard", "1.0 if a == 0.0", "same offset within its tile"):
        assert said in section, said
    for fn in ("saxs_profile", "ensemble_saxs", "hydrodynamic_radius", "saxs_mae", "mean_rh", "js_rh", "saxs_chi2", "read_saxs_dat"):
        assert callable(getattr(metrics, fn)), fn
    sig = inspect.signature(ops.ca_scattering).parameters
    assert list(sig) == ["ca", "q", "types", "table", "max_structures"] and all(sig[k].default is None for k in list(sig)[2:])
    assert list(inspect.signature(metrics.saxs_profile).parameters) == ["coords", "q", "aatype", "form_factors", "max_structures"]
    assert list(inspect.signature(metrics.ensemble_saxs).parameters)[:3] == ["coords", "q", "weights"]
    assert list(inspect.signature(metrics.saxs_chi2).parameters) == ["intensity", "i_exp", "sigma", "background"]
    assert metrics.SAXS_Q_GRID.tolist() == [k / 100.0 for k in range(51)]


def test_bad_sizes_are_invalid_value():
    """What the kernel cannot take is rejected before any launch (hipErrorInvalidValue = 1), so this needs no device."""
    from str2str_amd import build, ops

    if not os.path.exists(ops.LIB_PATH):
        build.build(verbose=False)
    lib = ops.load_library()
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(n=4, L=8, Q=6, T=1, ptrs=(p,) * 6):
        return lib.s2s_ca_scattering(ptrs[0], n, L, ptrs[1], Q, ptrs[2], ptrs[3], T, ptrs[4], ptrs[5], None)

    for kwargs in (dict(n=0), dict(n=-1), dict(L=0), dict(L=-3), dict(L=ops.SAXS_MAX_RES + 1), dict(Q=0), dict(Q=-2), dict(Q=ops.SAXS_MAX_Q + 1),
                   dict(T=0), dict(T=-1), dict(T=ops.SAXS_MAX_TYPES + 1)):
        assert call(**kwargs) == 1, kwargs
    for k in range(5):                                          # every buffer but inv_r_mean, which may be NULL
        assert call(ptrs=(p,) * k + (None,) + (p,) * (5 - k)) == 1, k


def test_argument_checks_fire_before_the_device(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics
    from str2str_amd.ops import ensemble

    def touched(*a, **k):
        raise AssertionError("touched the device")

    monkeypatch.setattr(ensemble, "load_library", touched)
    x = torch.zeros(4, 8, 3)
    q = [0.0, 0.1, 0.2]
    bad = [(dict(ca=torch.zeros(4, 8)), "ca"), (dict(ca=torch.zeros(4, 8, 2)), "ca"), (dict(ca=torch.zeros(0, 8, 3)), "ca"), (dict(ca=torch.zeros(4, 0, 3)), "ca"),
           (dict(ca=x.numpy()), "tensor"), (dict(ca=torch.zeros(1, ops.SAXS_MAX_RES + 1, 3)), "residues"),
           (dict(max_structures=0), "max_structures"), (dict(max_structures=1.5), "max_structures"), (dict(max_structures=True), "max_structures"),
           (dict(q=[]), "q"), (dict(q=[[0.1, 0.2]]), "q"), (dict(q=np.zeros(ops.SAXS_MAX_Q + 1)), "q"), (dict(q=[0.1, -0.1]), "q"),
           (dict(q=[0.1, float("nan")]), "q"), (dict(q=[0.1, float("inf")]), "q"), (dict(q=["a"]), "q"), (dict(q=[0.1 + 1j]), "q"),
           (dict(table=np.ones((2, 4))), "table"), (dict(table=np.ones(3)), "table"), (dict(table=np.ones((ops.SAXS_MAX_TYPES + 1, 3))), "table"),
           (dict(table=np.ones((0, 3))), "table"), (dict(table=np.array([[1.0, np.nan, 1.0]])), "table"), (dict(table=np.array([[1.0, np.inf, 1.0]])), "table"),
           (dict(types=np.zeros(7, dtype=int)), "types"), (dict(types=np.zeros(8)), "types"), (dict(types=np.ones(8, dtype=int)), "types"),
           (dict(types=-np.ones(8, dtype=int), table=np.ones((2, 3))), "types"), (dict(types=np.full(8, 2), table=np.ones((2, 3))), "types"),
           (dict(), "no CPU fallback"), (dict(types=torch.ones(8, dtype=torch.int64), table=torch.ones(2, 3)), "no CPU fallback"),
           (dict(ca=x.double()), "no CPU fallback")]
    for kwargs, match in bad:
        with pytest.raises(ops.HipLibraryError, match=match):
            ops.ca_scattering(**{**dict(ca=x, q=q), **kwargs})

    monkeypatch.setattr(metrics, "_dev", lambda v: torch.as_tensor(np.asarray(v)).float())
    for call, match in ((lambda: metrics.saxs_profile(np.zeros((4, 8, 3)), [[0.1]]), "q"), (lambda: metrics.saxs_profile(np.zeros((4, 8, 3)), []), "q"),
                        (lambda: metrics.saxs_profile(np.zeros((4, 8, 3)), q, form_factors=np.ones((2, 4))), "form_factors"),
                        (lambda: metrics.saxs_profile(np.zeros((4, 8, 3)), q, np.zeros(7, dtype=int), np.ones((2, 3))), "aatype")):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(ops.HipLibraryError, match="no CPU fallback"):
        metrics.hydrodynamic_radius(np.zeros((4, 8, 3)))


# ------------------------------------------------------------------------------------------------------- the numpy tails of the metrics
def yardstick_as_device(monkeypatch):
    """``ops.ca_scattering`` answered by the yardstick on host tensors, so that everything after the kernel runs without a device."""
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    calls = []

    def fake(ca, q, types=None, table=None, max_structures=None):
        calls.append(len(q))
        return tuple(torch.from_numpy(v) for v in ref.scattering(ca.numpy(), q, types, table))

    monkeypatch.setattr(ops, "ca_scattering", fake)
    monkeypatch.setattr(metrics, "_dev", lambda a: (torch.as_tensor(np.array(a))[None] if np.ndim(a) == 2 else torch.as_tensor(np.array(a))).float().contiguous())
    return calls


def test_ensemble_metrics_are_the_plain_numpy_tails(monkeypatch):
    from str2str_amd import ops
    from str2str_amd.metrics import metrics

    calls = yardstick_as_device(monkeypatch)
    c = cases.case("L13_R17_T3")
    both = {"target": c.ca[:9], "pred": c.ca[6:], "same": c.ca[:9].copy()}
    q = metrics.SAXS_Q_GRID
    want = {k: ref.scattering(v, q) for k, v in both.items()}
    rows = metrics.saxs_profile(both["pred"], q)
    assert rows.dtype == np.float64 and rows.tobytes() == want["pred"][0].tobytes()
    assert metrics.saxs_profile(both["pred"][2], q).tobytes() == want["pred"][0][2:3].tobytes()      # a single structure without the leading axis
    typed = metrics.saxs_profile(both["pred"], c.q, c.types, c.table)
    assert typed.tobytes() == ref.scattering(both["pred"], c.q, c.types, c.table)[0].tobytes()
    assert metrics.saxs_profile(both["pred"], c.q, c.types).tobytes() == ref.scattering(both["pred"], c.q)[0].tobytes()   # no table: the types are not used
    mean = metrics.ensemble_saxs(both["pred"], q)
    assert mean.shape == (51,) and (mean == want["pred"][0].mean(0)).all() and mean[0] == 169.0
    w = np.linspace(0.5, 2.0, len(both["pred"]))
    assert (metrics.ensemble_saxs(both["pred"], q, w) == np.average(want["pred"][0], axis=0, weights=w)).all()
    with pytest.raises(ValueError, match="weights"):
        metrics.ensemble_saxs(both["pred"], q, w[:-1])
    rh = {k: 1.0 / v[1] for k, v in want.items()}
    assert (metrics.hydrodynamic_radius(both["pred"]) == rh["pred"]).all() and (rh["pred"] > 0).all()

    curve = {k: v[0].mean(0) for k, v in want.items()}
    mae = metrics.saxs_mae(both)
    assert mae["target"] == 0.0 and mae["same"] == 0.0
    assert mae["pred"] == np.around(float((np.abs(curve["pred"] - curve["target"]) / curve["target"]).mean()), decimals=4) > 0.0
    weights = {"pred": w}
    curve_w = np.average(want["pred"][0], axis=0, weights=w)
    assert metrics.saxs_mae(both, weights=weights)["pred"] == np.around(float((np.abs(curve_w - curve["target"]) / curve["target"]).mean()), decimals=4)
    short = metrics.saxs_mae(both, q=[0.0, 0.2])
    assert short["pred"] == np.around(float((np.abs(curve["pred"] - curve["target"]) / curve["target"])[[0, 20]].mean()), decimals=4)
    mrh = metrics.mean_rh(both)
    assert mrh == {k: np.around(float(v.mean()), decimals=4) for k, v in rh.items()} and mrh["pred"] != mrh["target"]
    assert metrics.mean_rh(both, weights=weights)["pred"] == np.around(float(np.average(rh["pred"], weights=w)), decimals=4)
    lo, hi = rh["target"].min(), rh["target"].max()
    hist = {k: np.histogram(v, bins=50, range=(lo, hi))[0] + metrics.PSEUDO_C for k, v in rh.items()}
    js = metrics.js_rh(both)
    assert js["target"] == 0.0 and js["same"] == 0.0 and js["pred"] == np.around(metrics._js(hist["pred"], hist["target"]), decimals=4) and 0.0 < js["pred"] < 1.0
    hist_w = np.histogram(rh["pred"], bins=12, weights=w, range=(lo, hi))[0] + metrics.PSEUDO_C
    hist_t = np.histogram(rh["target"], bins=12, range=(lo, hi))[0] + metrics.PSEUDO_C
    assert metrics.js_rh(both, n_bins=12, weights=weights)["pred"] == np.around(metrics._js(hist_w, hist_t), decimals=4)
    with pytest.raises(ValueError, match="weights"):
        metrics.js_rh(both, weights={"pred": w[:-1]})

    # a q-list longer than one call takes is walked in runs of whole tiles
    del calls[:]
    long_q = np.linspace(0.0, 0.5, ops.SAXS_MAX_Q + 40)
    rows = metrics.saxs_profile(both["pred"][:2], long_q)
    assert calls == [ops.SAXS_MAX_Q, 40] and ops.SAXS_MAX_Q % 16 == 0 and rows.tobytes() == ref.scattering(both["pred"][:2], long_q)[0].tobytes()


# ------------------------------------------------------------------------------------------------------- the fit to a measured curve
@pytest.mark.parametrize("background", (False, True))
def test_saxs_chi2_against_lstsq(background):
    from str2str_amd.metrics import metrics

    rng = np.random.default_rng(5)
    q = np.linspace(0.01, 0.5, 40)
    i_calc = ref.scattering(cases.case("L31_R9").ca[:1], q)[0][0]
    sigma = 0.5 + 0.02 * np.sqrt(i_calc) * rng.uniform(0.5, 1.5, size=len(q))
    scale, const = 3.75e-3, (0.8 if background else 0.0)
    noise = rng.normal(size=len(q))
    i_exp = scale * i_calc + const + sigma * noise
    chi2, got_scale, got_const = metrics.saxs_chi2(i_calc, i_exp, sigma, background)
    A = np.stack([i_calc / sigma] + ([1.0 / sigma] if background else []), axis=1)
    sol, res, _, _ = np.linalg.lstsq(A, i_exp / sigma, rcond=None)
    dof = len(q) - (2 if background else 1)
    assert abs(got_scale - sol[0]) <= 1e-10 * abs(sol[0]) and abs(chi2 - float(res[0]) / dof) <= 1e-9 * chi2
    assert (abs(got_const - sol[1]) <= 1e-9 * abs(sol[1])) if background else got_const == 0.0
    # without noise the planted scale (and constant) come back and chi^2 vanishes
    chi2_0, scale_0, const_0 = metrics.saxs_chi2(i_calc, scale * i_calc + const, sigma, background)
    assert abs(scale_0 - scale) <= 1e-12 * scale and abs(const_0 - const) <= 1e-9 and chi2_0 <= 1e-18
    # the chi^2 of the planted noise: what the fit leaves of it is the noise less its projection onto the fitted columns
    planted = float((noise * noise).sum())
    inside = A @ np.linalg.lstsq(A, noise, rcond=None)[0]
    assert abs(chi2 * dof - (planted - float((inside * inside).sum()))) <= 1e-9 * planted and chi2 * dof <= planted
    assert 0.3 < chi2 < 3.0


def test_saxs_chi2_rejects_bad_curves():
    from str2str_amd.metrics import metrics

    ok = np.ones(5)
    for args in ((ok, ok[:4], ok), (ok, ok, ok[:4]), (np.ones((5, 1)), ok, ok), (ok[:1], ok[:1], ok[:1]), (ok, ok, np.zeros(5)), (ok, ok, -ok),
                 (ok, ok, np.full(5, np.nan))):
        with pytest.raises(ValueError, match="saxs_chi2"):
            metrics.saxs_chi2(*args)
    with pytest.raises(ValueError, match="saxs_chi2"):
        metrics.saxs_chi2(ok[:2], ok[:2], ok[:2], background=True)


def test_read_saxs_dat(tmp_path):
    from str2str_amd.metrics import metrics

    path = tmp_path / "curve.dat"
    path.write_text("Sample: lysozyme 5 mg/ml\n"
                    "# q(1/nm)  I(q)  error\n"
                    "   q   I   sigma\n"
                    "0.10  1.50e+02  2.0\n"
                    "0.20\t1.25e+02\t1.5   # a trailing remark\n"
                    "\n"
                    "0.30  9.0e+01  0.0\n"                      # sigma = 0: dropped
                    "0.35  8.0e+01  -1.0\n"                     # sigma < 0: dropped
                    "0.40  7.0e+01  1.0  extra\n"               # four fields: skipped
                    "# 0.45 6.0e+01 1.0\n"
                    "0.50  5.0e+01  0.5\n"
                    "creator: beamline software 1.2 3\n"
                    "end of data\n")
    q, i, s = metrics.read_saxs_dat(str(path), q_unit="1/nm")
    assert all(a.dtype == np.float64 for a in (q, i, s))
    assert q.tolist() == [0.10 / 10.0, 0.20 / 10.0, 0.50 / 10.0] and i.tolist() == [150.0, 125.0, 50.0] and s.tolist() == [2.0, 1.5, 0.5]
    assert metrics.read_saxs_dat(str(path))[0].tolist() == [0.10, 0.20, 0.50]
    with pytest.raises(ValueError, match="q_unit"):
        metrics.read_saxs_dat(str(path), q_unit="nm")
    empty = tmp_path / "empty.dat"
    empty.write_text("# nothing\n")
    assert [len(a) for a in metrics.read_saxs_dat(str(empty))] == [0, 0, 0]
