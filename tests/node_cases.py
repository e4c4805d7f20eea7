"""Seeded case table of the node-stream parity suite (tests/test_node_parity.py, tests/test_node_parity_cpu.py), its measure and
its bound rule.  Nothing here looks at a kernel.

Row counts ``ROWS``: 1, 31, 32, 33 (around one 32-row tile), 127, 129 (around one 128-row workgroup), 257, 5 x 128 + 40 (several
workgroups and a ragged last tile).  Padded row maps ``ROW_MAPS`` (n_pad, n_src) for N = 1, 33, 75.

Families (of single layers, ``layer_case``, and of a block's stages, ``stage_inputs``):
  flat          inputs and residuals N(0, 1), weights of synth_sd(0, 0.02)
  trained-like  synth_state_dict(style="trained_like") weights, inputs x 150: hidden activations of thousands, below 2^15 (x 30 gives
                only a few hundred with these weights)
  offset        every row in front of a LayerNorm is c_row + N(0, 1), |c_row| up to 30
  small         row r of the plane-format input carries the scale 2^-(r mod 16); single layers also with the whole weight matrix
                x 1, 2^-6, 2^-10 (and no bias: a bias would set the scale of the row and hide the product)
  masked        pre / post / diffuse masks with isolated zeros, a zero prefix, all zero (by row count); residual rows zero where the
                trunk would have masked them; rows whose every value in front of a ReLU is negative

Measure, per valid row:  max_c |got - float64| / scale_row, the error of a (case, output) its maximum over the rows; no floor.
  scale_row = max_c |float64|                                     behind a LayerNorm
            = max_c (sum_k |x_rk| |w_ck| |pre_scale_r| + |b_c| + |res_rc|)   behind a linear layer: its forward-error scale
Rows that must be exact (post_mask 0 -> 0; pre_mask 0 and residual 0 in front of a LayerNorm -> beta) are not pooled: ``exact_rows``.

Bound of a (family, output):  3 x D32 + F.
  D32  distance of ref_node in float32 from float64 under the same measure, pooled (max) over ``ROWS``; flat and offset: at most 5e-6.
  F    f16x3 only, per row, derived from the format and not measured.  A plane pair (t_h, t_l) = (rn16(t), rn16(t - t_h)) has a low
       plane below f16's normal range (2^-14), where f16 rounds to 2^-25 absolute, for |t| < 0.25; weights are split as 32 w, so their
       low plane is there for |w| < 2^-8 and the error is 2^-30 in units of w.  Hence per output element
           2^-25 sum_{k: 0 < |x_rk| < 0.25} |w_ck|  +  2^-30 sum_{k: 0 < |w_ck| < 2^-8} |x_rk|,
       through the layer's epilogue (pre_scale, masks, the LayerNorm's derivative), each layer's floor taken through the later layers'
       |W|, divided by scale_row.  Larger elements keep relative 2^-24: the float32 chain's own rounding, inside D32.
"""
import functools

import torch

import ref_node as RN
from conftest import manifest, synth_sd

ROWS = (1, 31, 32, 33, 127, 129, 257, 5 * 128 + 40)
ROW_MAPS = {1: (32, 1), 33: (64, 33), 75: (96, 75)}
FAMILIES = ("flat", "trained-like", "offset", "small", "masked")
W_SCALES = (1.0, 2.0 ** -6, 2.0 ** -10)
CAP = 5e-6
AMP_TRAINED = 150.0
OFFSET = 30.0
X_LOW, W_LOW, EPS_X, EPS_W = 0.25, 2.0 ** -8, 2.0 ** -25, 2.0 ** -30
T = RN.TRUNK

# single layers of block 0: name -> (weights, LayerNorm or None, how the trunk runs it)
KINDS = {"skip": (T + "skip_embed_0", None, "plain"),                       # 256 -> 64, final-initialised
         "in_proj": (T + "transformer_0.layers.0.self_attn.in_proj", None, "plain"),   # 320 -> 960
         "linear_out": (T + "ipa_0.linear_out", T + "ipa_ln_0", "pre_mask"),   # 2688 -> 256: mask, residual, LayerNorm
         "nt3": (T + "node_transition_0.linear_3", T + "node_transition_0.ln", "post_mask"),   # 256 -> 256: residual, LayerNorm, mask
         "l1": (T + "transformer_0.layers.0.linear1", None, "relu"),           # 320 -> 320, ReLU
         "l2": (T + "transformer_0.layers.0.linear2", T + "transformer_0.layers.0.norm2", "residual"),   # 320 -> 320: residual, LayerNorm
         "bb": (T + "bb_update_0.linear", None, "pre_scale")}                  # 256 -> 6 (padded to 32 columns), diffuse mask as pre_scale
LN_KINDS = tuple(k for k, v in KINDS.items() if v[1])


@functools.lru_cache(maxsize=None)
def trained_sd():
    from str2str_amd.synth import synth_state_dict

    return synth_state_dict(manifest(), seed=0, sigma_final=0.02, style="trained_like")


def sd_of(family):
    return trained_sd() if family == "trained-like" else synth_sd(0, 0.02)


def mask_pattern(M, g, kind=None):
    """By row count (or ``kind`` 0 | 1 | 2): isolated zeros | a zero prefix | all zero."""
    if kind is None:
        kind = ROWS.index(M) % 3 if M in ROWS else 0
    m = torch.ones(M)
    if kind == 0:
        m = (torch.rand(M, generator=g) >= 0.3).float()
        if M > 1:
            m[0], m[M - 1] = 1.0, 0.0
    elif kind == 1:
        m[:(M + 1) // 2] = 0
    else:
        m[:] = 0
    return m


def row_scales(M):
    return 2.0 ** -(torch.arange(M) % 16).float()


def _weights(family, kind):
    p, ln, _ = KINDS[kind]
    sd = sd_of(family)
    w = sd[p + ".weight"] if p + ".weight" in sd else sd[p + "_weight"]
    b = sd[p + ".bias"] if p + ".bias" in sd else sd[p + "_bias"]
    return w, b, (RN.ln_of(sd, ln) if ln else None)


@functools.lru_cache(maxsize=None)
def layer_case(family, kind, M, w_scale=1.0):
    """-> dict(name, family, kind, M, kw = the arguments of ref_node.layer, fp32 tensors on the CPU).  Do not modify."""
    w, b, ln = _weights(family, kind)
    how = KINDS[kind][2]
    n, K = w.shape
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(family) + 37 * M + sorted(KINDS).index(kind))
    amp = AMP_TRAINED if family == "trained-like" else 1.0
    x = amp * torch.randn(M, K, generator=g)
    kw = dict(x=x, w=w, b=b, ln=ln)
    if ln is not None:
        kw["residual"] = amp * torch.randn(M, n, generator=g)
    if how == "relu":
        kw["relu"] = True
    if how == "pre_scale":
        kw["pre_scale"] = (torch.rand(M, generator=g) >= 0.3).float()
    if family == "small":
        kw = dict(x=x * row_scales(M)[:, None], w=(w * w_scale).contiguous(), b=None, relu=how == "relu", ln=None)
    if family == "offset" and ln is not None:
        c = OFFSET * (2 * torch.rand(M, 1, generator=g) - 1)
        v0 = RN.layer(x, w, b, relu=kw.get("relu", False))
        kw["residual"] = (c.double() + torch.randn(M, n, generator=g).double() - v0).float()
    if family == "masked":
        m = mask_pattern(M, g)
        if how == "pre_mask":
            kw["pre_mask"] = m
            kw["residual"] = kw["residual"] * m[:, None]
        elif how == "post_mask":
            kw["post_mask"] = m
        elif how == "pre_scale":
            kw["pre_scale"] = m
        elif how == "relu":       # rows of zeros under an all-negative bias: every value in front of the ReLU is negative
            kw["x"] = x * m[:, None]
            kw["b"] = -b.abs() - 1e-3
        elif how == "residual":
            kw["pre_mask"] = m
    return dict(name=f"{family}-{kind}-M{M}" + (f"-w{w_scale:g}" if w_scale != 1.0 else ""), family=family, kind=kind, M=M, kw=kw)


# ---------------------------------------------------------------------------------------------------- the measure
def record_scale(rec):
    """[M] float64: scale_row of a trace record (ref_node.layer, evaluated in float64)."""
    if rec["ln"] is not None:
        return rec["out"].abs().amax(-1)
    s = rec["x"].abs() @ rec["w"].abs().t()
    if rec["pre_scale"] is not None:
        s = s * rec["pre_scale"].abs()[:, None]
    if rec["b"] is not None:
        s = s + rec["b"].abs()
    if rec["residual"] is not None:
        s = s + rec["residual"][:, :s.shape[1]].abs()
    return s.amax(-1)


def exact_rows(rec):
    """-> (rows [M] bool, expected [M, n] float64): the rows of a record's output that every correct evaluation gives exactly."""
    M, n = rec["out"].shape
    rows = torch.zeros(M, dtype=torch.bool, device=rec["out"].device)
    want = torch.zeros(M, n, dtype=torch.float64, device=rec["out"].device)
    if rec["ln"] is not None and rec["pre_mask"] is not None:
        dead = rec["pre_mask"] == 0
        if rec["residual"] is not None:
            dead = dead & (rec["residual"][:, :n] == 0).all(-1)
        rows |= dead
        want[dead] = rec["ln"][1].to(want)
        if rec["post_mask"] is not None:
            want = want * rec["post_mask"][:, None]
    if rec["post_mask"] is not None:
        z = rec["post_mask"] == 0
        rows |= z
        want[z] = 0
    return rows, want


def row_errors(got, rec):
    """[M] float64: max_c |got - float64| / scale_row; nan on rows without a scale (exact rows, rows of zeros)."""
    ref = rec["out"]
    err = (got.to(ref.device).double() - ref).abs().amax(-1)
    scale = record_scale(rec)
    ok = (scale > 0) & ~exact_rows(rec)[0]
    return torch.where(ok, err / scale.clamp_min(1e-300), torch.full_like(err, float("nan")))


def unscaled_rows(rec):
    """[M] bool: rows without a scale that are not among the exact rows (a row of zeros through a layer without bias and residual).
    Their float64 output is zero, and so must every evaluation's be."""
    return (record_scale(rec) == 0) & ~exact_rows(rec)[0]


def nanmax(t):
    t = t[~torch.isnan(t)]
    return float(t.max()) if t.numel() else 0.0


def floors(trace):
    """Per record of a float64 trace: [M, n] absolute error bound of the f16x3 format (module docstring), earlier layers' floors
    taken along (a record's ``x`` / ``residual`` that IS an earlier record's output carries that output's floor; so does an ``x`` that
    is the sum of an earlier output, named by the record's ``x_from``, and a given tensor).  A record's ``exp`` = e scales the
    activation term: planes of 2^-e x the value round to 2^(e-25) below 2^e x 0.25."""
    err, out = {}, []
    for rec in trace:
        x, w = rec["x"], rec["w"]
        ax, aw = x.abs(), w.abs()
        n = w.shape[0]
        k = 2.0 ** rec.get("exp", 0)      # a block exponent e: the planes hold 2^-e x the value (tests/ref_pair.py)
        f = k * EPS_X * (((ax < k * X_LOW) & (ax > 0)).double() @ aw.t()) + EPS_W * (ax @ ((aw < W_LOW) & (aw > 0)).double().t())
        src = rec.get("x_from", x)        # an input that is an earlier output PLUS a given tensor carries that output's floor
        if id(src) in err:
            f = f + err[id(src)] @ aw.t()
        for t, idx, c0 in rec.get("x_add_from", ()):      # ... and a given tensor that is rows ``idx`` of an earlier output, at columns c0..
            if id(t) in err:
                f = f + err[id(t)][idx] @ aw[:, c0:c0 + err[id(t)].shape[1]].t()
        for t, idx in rec.get("b_from", ()):              # a per-row bias gathered from rows ``idx`` of an earlier output
            if id(t) in err:
                f = f + err[id(t)][idx]
        if rec["pre_scale"] is not None:
            f = f * rec["pre_scale"].abs()[:, None]
        if rec["pre_mask"] is not None:
            f = f * rec["pre_mask"].abs()[:, None]
        if rec["residual"] is not None and id(rec["residual"]) in err:
            f = f + err[id(rec["residual"])][:, :n]
        if rec["ln"] is not None:
            # y_c = g_c vhat_c + beta, vhat = (v - mean) / sd.  To first order  dy_c = g_c / sd (dv_c - dmean - vhat_c dsd)  with
            # dsd = mean_j vhat_j (dv_j - dmean), so  |dy_c| <= |g_c| / sd (e_c + mean e + |vhat_c| mean_j |vhat_j| (e_j + mean e))
            v = rec["pre_ln"]
            sd = torch.sqrt(v.var(dim=-1, unbiased=False, keepdim=True) + rec["ln"][2])
            vhat = (v - v.mean(-1, keepdim=True)).abs() / sd
            fc = f + f.mean(-1, keepdim=True)
            f = rec["ln"][0].to(f).abs() / sd * (fc + vhat * (vhat * fc).mean(-1, keepdim=True))
        if rec["post_mask"] is not None:
            f = f * rec["post_mask"].abs()[:, None]
        err[id(rec["out"])] = f
        out.append(f)
    return out


def row_floor(trace, i=-1):
    """[M]: F of record ``i`` of a float64 trace, per row (0 where the row has no scale)."""
    f = floors(trace)[i].amax(-1)
    scale = record_scale(trace[i])
    return torch.where(scale > 0, f / scale.clamp_min(1e-300), torch.zeros_like(f))


def check_rows(got, rec, d32, floor=None, cap=False):
    """-> (achieved, bound, worst row) of ``got`` against a float64 record: the row with the largest error / bound, where the bound of
    a row is 3 x D32 (capped) + its F."""
    e = row_errors(got, rec)
    base = min(3.0 * d32, CAP) if cap else 3.0 * d32
    b = torch.full_like(e, base) if floor is None else base + floor.to(e)
    ratio = torch.where(torch.isnan(e), torch.zeros_like(e), e / b)
    r = int(ratio.argmax())
    if torch.isnan(e[r]):
        return 0.0, float(b[r]), r
    return float(e[r]), float(b[r]), r


def capped(family):
    return family in ("flat", "offset")


# ---------------------------------------------------------------------------------------------------- single layers: reference, D32
@functools.lru_cache(maxsize=None)
def layer_ref(family, kind, M, w_scale=1.0):
    """The float64 trace (one record) of a single-layer case.  Shared; do not modify."""
    tr = []
    RN.layer(**layer_case(family, kind, M, w_scale)["kw"], dtype=torch.float64, trace=tr)
    return tr


@functools.lru_cache(maxsize=None)
def layer_d32(family, kind, w_scale=1.0):
    """D32 of a (family, single layer): float32 against float64, pooled over ROWS."""
    return max(nanmax(row_errors(RN.layer(**layer_case(family, kind, M, w_scale)["kw"], dtype=torch.float32), layer_ref(family, kind, M, w_scale)[0]))
               for M in ROWS)


def layer_kinds(family):
    return LN_KINDS if family == "offset" else tuple(KINDS)


def layer_table():
    """Every (family, kind, w_scale) of the single-layer table (each over ROWS)."""
    return [(f, k, ws) for f in FAMILIES for k in layer_kinds(f) for ws in (W_SCALES if f == "small" else (1.0,))]


# ---------------------------------------------------------------------------------------------------- a block's stages
STAGES = ("linear_out", "skip_embed", "in_proj", "post_attention", "node_transition", "backbone_update", "edge_node_parts", "torsion_head")
# outputs of a stage: name -> index of its record in the stage's trace
OUTPUTS = {"linear_out": {"x_ln": 0}, "skip_embed": {"skip": 0}, "in_proj": {"qkv": 0}, "post_attention": {"x1": 0, "x2": 2},
           "node_transition": {"n": 0, "s1": 3}, "backbone_update": {"upd": 0}, "edge_node_parts": {"n_p": 0, "A": 1, "B": 2, "G": 3},
           "torsion_head": {"u": 2}}


@functools.lru_cache(maxsize=None)
def stage_inputs(family, M, B=None):
    """Inputs of every stage of block 0 at M rows (independent draws: a stage is tested from given inputs, not from the stage in
    front of it).  The plane-format inputs (feats, init, x, sa, s1) carry the family's amplitude / row scales; the residual inputs
    (s, x as residual) the family's offset.  Do not modify."""
    g = torch.Generator().manual_seed(50000 + 100 * FAMILIES.index(family) + M)
    amp = AMP_TRAINED if family == "trained-like" else 1.0
    r = lambda c: amp * torch.randn(M, c, generator=g)  # noqa: E731
    d = dict(feats=r(2688), s=r(256), init=r(256), x=r(320), sa=r(320), s1=r(256), gt=torch.randn(M, 2, generator=g))
    d["gt"] = d["gt"] / d["gt"].norm(dim=-1, keepdim=True)
    d["mask"], d["fixed"] = torch.ones(M), torch.zeros(M)
    if family == "small":
        for k in ("feats", "init", "sa", "s1"):
            d[k] = d[k] * row_scales(M)[:, None]
        d["x_act"] = d["x"] * row_scales(M)[:, None]
    if family == "offset":
        c = OFFSET * (2 * torch.rand(M, 1, generator=g) - 1)
        d["s"], d["x"] = d["s"] + c, d["x"] + c
    if family == "masked":
        d["mask"] = mask_pattern(M, g)
        d["fixed"] = (torch.rand(M, generator=g) < 0.4).float()
        for k in ("s", "s1"):
            d[k] = d[k] * d["mask"][:, None]
    d.setdefault("x_act", d["x"])
    d["diffuse"] = (1 - d["fixed"]) * d["mask"]
    return d


def run_stage(stage, sd, d, dtype=torch.float64, L=RN.layer):
    """Stage ``stage`` of block 0 on the inputs ``d`` -> (outputs {name: tensor}, trace)."""
    tr = []
    kw = dict(dtype=dtype, L=L, trace=tr)
    if stage == "linear_out":
        RN.linear_out(sd, 0, d["feats"], d["s"], d["mask"], **kw)
    elif stage == "skip_embed":
        RN.skip_embed(sd, 0, d["init"], **kw)
    elif stage == "in_proj":
        RN.in_proj(sd, 0, 0, d["x_act"], **kw)
    elif stage == "post_attention":
        RN.post_attention(sd, 0, 0, d["x"], d["sa"], **kw)
    elif stage == "node_transition":
        RN.node_transition(sd, 0, d["s"], d["x_act"], d["mask"], **kw)
    elif stage == "backbone_update":
        RN.backbone_update(sd, 0, d["s1"], d["diffuse"], **kw)
    elif stage == "edge_node_parts":
        RN.edge_node_parts(sd, 0, d["s1"], **kw)
    elif stage == "torsion_head":
        RN.torsion_head(sd, d["s1"], d["gt"], d["fixed"], **kw)
    else:
        raise KeyError(stage)
    return {name: tr[i]["out"] for name, i in OUTPUTS[stage].items()}, tr


@functools.lru_cache(maxsize=None)
def stage_ref(family, stage, M):
    """(outputs, trace) of a stage in float64.  Shared; do not modify."""
    return run_stage(stage, sd_of(family), stage_inputs(family, M))


@functools.lru_cache(maxsize=None)
def stage_d32(family, stage):
    """{output: D32} of a (family, stage), pooled over ROWS."""
    out = {name: 0.0 for name in OUTPUTS[stage]}
    for M in ROWS:
        got, _ = run_stage(stage, sd_of(family), stage_inputs(family, M), dtype=torch.float32)
        _, tr = stage_ref(family, stage, M)
        for name, i in OUTPUTS[stage].items():
            out[name] = max(out[name], nanmax(row_errors(got[name], tr[i])))
    return out


# ---------------------------------------------------------------------------------------------------- a LayerNorm on its own
def ln_record(x, ln, dtype=torch.float64):
    """A trace record of LayerNorm(x) alone (s2s_row_layernorm), x as the float32 rows the kernel reads."""
    v = x.to(dtype)
    out = RN.layer_norm(v, ln[0].to(v), ln[1].to(v), ln[2])
    return dict(x=None, w=None, b=None, pre_scale=None, relu=False, pre_mask=None, residual=None, ln=ln, post_mask=None, pre_ln=v, out=out)


@functools.lru_cache(maxsize=None)
def ln_case(kind, M):
    """(x [M, n] float32, ln): the rows in front of the LayerNorm of the offset family's layer ``kind``, rounded to float32."""
    return layer_ref("offset", kind, M)[0]["pre_ln"].float(), layer_case("offset", kind, M)["kw"]["ln"]


@functools.lru_cache(maxsize=None)
def ln_d32(kind):
    return max(nanmax(row_errors(ln_record(*ln_case(kind, M), dtype=torch.float32)["out"], ln_record(*ln_case(kind, M)))) for M in ROWS)


# ---------------------------------------------------------------------------------------------------- chains of square layers
# name -> (width, [(weights, relu)], LayerNorm behind the last layer (with a residual) or None)
CHAINS = {"2x256": (256, [(T + "node_transition_0.linear_1", True), (T + "node_transition_0.linear_2", True)], None),
          "3x256": (256, [(T + "node_transition_0.linear_1", True), (T + "node_transition_0.linear_2", True),
                          (T + "node_transition_0.linear_3", False)], T + "node_transition_0.ln"),
          "2x320": (320, [(T + "transformer_0.layers.0.linear1", True), (T + "transformer_0.layers.0.linear2", False)],
                    T + "transformer_0.layers.0.norm2"),
          "4x320": (320, [(T + "transformer_0.layers.0.self_attn.out_proj", False), (T + "transformer_0.layers.0.linear1", True),
                          (T + "transformer_0.layers.1.linear1", True), (T + "transformer_0.layers.0.linear2", False)],
                    T + "transformer_0.layers.0.norm2")}
CHAIN_FAMILIES = FAMILIES      # (offset: on the chains that end in a LayerNorm)


@functools.lru_cache(maxsize=None)
def chain_inputs(family, name, M):
    width = CHAINS[name][0]
    g = torch.Generator().manual_seed(70000 + 100 * FAMILIES.index(family) + M + width)
    amp = AMP_TRAINED if family == "trained-like" else 1.0
    x, res = amp * torch.randn(M, width, generator=g), amp * torch.randn(M, width, generator=g)
    if family == "small":
        x = x * row_scales(M)[:, None]
    if family == "offset":
        res = res + OFFSET * (2 * torch.rand(M, 1, generator=g) - 1)
    mask = mask_pattern(M, g) if family == "masked" else None
    return x, res, mask


def run_chain(name, sd, x, res, mask, dtype=torch.float64, L=RN.layer):
    """-> trace of the chain: relu?(W x + b) per layer; the last with the residual, the LayerNorm and the mask behind it."""
    _, layers, ln = CHAINS[name]
    tr, act = [], x
    for i, (p, relu) in enumerate(layers):
        last = i == len(layers) - 1
        kw = dict(residual=res, ln=RN.ln_of(sd, ln), post_mask=mask) if last and ln else {}
        act = L(act, *RN.lin(sd, p), relu=relu, dtype=dtype, trace=tr, **kw)
    return tr


@functools.lru_cache(maxsize=None)
def chain_d32(family, name):
    return max(nanmax(row_errors(run_chain(name, sd_of(family), *chain_inputs(family, name, M), dtype=torch.float32)[-1]["out"],
                                 run_chain(name, sd_of(family), *chain_inputs(family, name, M))[-1])) for M in ROWS)


# ---------------------------------------------------------------------------------------------------- psi
def psi_errors(got, u_rec, gt, fixed, floor_u=None):
    """-> (errors [M], floors [M]) of psi = blend(u / |u|) against float64: |got - psi64| per row (|psi| <= 1 is its own scale), and
    the floor of u taken through the normalisation (|d psi| <= 2 |d u| / |u|, nothing on fixed rows)."""
    u = u_rec["out"]
    psi = RN.torsion_normalise(u, gt.to(u.device), fixed.to(u.device))
    err = (got.to(u.device).double() - psi).abs().amax(-1)
    free = 1 - fixed.to(u)
    fl = torch.zeros_like(err) if floor_u is None else 2 * floor_u.amax(-1) / u.norm(dim=-1).clamp_min(1e-4) * free
    return err, fl


@functools.lru_cache(maxsize=None)
def psi_d32(family):
    worst = 0.0
    for M in ROWS:
        d = stage_inputs(family, M)
        _, tr = stage_ref(family, "torsion_head", M)
        u32 = RN.torsion_head(sd_of(family), d["s1"], dtype=torch.float32)[0]
        psi32 = RN.torsion_normalise(u32, d["gt"], d["fixed"], dtype=torch.float32)
        worst = max(worst, float(psi_errors(psi32, tr[2], d["gt"], d["fixed"])[0].max()))
    return worst
