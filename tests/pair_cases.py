"""Seeded case table of the pair-stream parity suite (tests/test_pair_parity.py, tests/test_pair_parity_cpu.py), its measure and its
bound rule.  Nothing here looks at a kernel.

Shapes (B, N), each the smallest that reaches its path of s2s_edge_transition_f16x3 (csrc/edge_transition_f16.h):
  N < 32 (the short-chain instantiation)   (1, 1), (1, 2), (3, 7) = 147 pairs: a partial second 128-pair tile, a partial 32-pair block, (2, 31)
  N >= 32                                  (1, 32), (1, 33), (2, 37)
  launch splits under S2S_ET_MAX_PAIRS     (5, 24) in launches of 2 + 2 + 1 samples, (20, 6) with a budget of 10 samples lowered to 8
  more tiles than persistent workgroups    (1, 190): 36 100 pairs = 283 tiles on 256 CUs, the last tile holds 4 pairs

Families (block 0's EdgeTransition, the projection of IPA block 1):
  flat          s, edge N(0, 1), weights of synth_sd(0, 0.02), no mask argument
  trained-like  node_cases.trained_sd(), inputs x 150: hidden activations of thousands, below 2^15
  offset-G      operator level: G_j + c_j on all 128 columns, |channel mean of y| up to 30 x the pair's own channel spread (std of y)
  offset-W      module level: final_layer.bias + c and final_layer.weight + 1 v^T on a copy, so that the offset varies per pair
  small         edge row of pair p x 2^-(p mod 16), node row r x 2^-(r mod 16), no bias in front of the LayerNorm (a bias would set the
                row's scale and hide the product)
  masked        node masks by shape (isolated zeros | a zero prefix | all zero); b2 negative and one residue whose A_i is -1000 on every
                channel at the operator level: all its pairs have every layer-1 and layer-2 pre-activation negative
  exp5/10/15    block exponent e: trunk.0 (and, beyond what its f16 packing takes, the inputs) scaled on a copy so that the largest
                hidden activation is 2^(13.5+e); the other weights keep their ordinary size.  Inputs and n' stay
                below 2^14 (the planes of the edge row and of the node stream carry no exponent), which at e = 15 leaves the hidden
                maximum near 2^27: the largest that admissible inputs reach, and 2^7 beyond what e - 5 takes

Measure, per valid pair, no floor:  max_c |got - float64| / scale_pair,
  scale_pair = max_c |out64_c - beta_c|                   for out (the normalised row without the LayerNorm's shift)
             = max_c (sum_k |z64_k| |w_ck| + |b_c|)       for attn_bias | pair_z (node_cases.record_scale)
Masked pairs are exact (out 0, projections = their bias as the reference computes it) and are not pooled.

Bound of a pair of a (family, level, output), arith "f16x3":  3 x D32 + min(1, 3 x r16) x F_pair;  arith "f32": 3 x D32.
  D32   the distance of ref_pair in float32 (ref_node.matmul: the plain loop over k) from float64 under the same measure, pooled over
        SHAPES; 3 x D32 capped at node_cases.CAP for flat and offset-*.
  F     the f16x3 format's a-priori worst case per pair (node_cases.floors; with a block exponent e the activation term of the layers
        that read hidden activations is 2^(e-25)).  It adds every sub-normal low-plane rounding with one sign and takes the sum through
        |W| of every later layer and the LayerNorm's derivative: chained over four (parts) or eight (module) layers it is hundreds of
        times what the format loses, and on its own hides a whole dropped low plane.  It keeps the SHAPE of the bound: it follows the
        2^-(p mod 16) scale classes of ``small`` and the block exponent.
  r16   how much of F the format really uses (``r16``): the largest error / F_pair of the faithful CPU emulation of the planes
        (``emulation``: the three plane products accumulated in float64, so the format's loss alone) over every valid pair of
        SMALL_SHAPES, per (family, level, output).  Measured on the test-side emulation only, never on a kernel.  The factor 3 is the
        one D32 carries, for the same reason (a kernel sums in another order than the reference of the figure); min(1, .) keeps the
        rule from ever being looser than 3 x D32 + F.  The level is read off the float64 trace (``level_of``).
"""
import functools

import torch

import node_cases as NC
import ref_node as RN
import ref_pair as RP
from conftest import synth_sd

SHAPES = ((1, 1), (1, 2), (3, 7), (2, 31), (1, 32), (1, 33), (2, 37), (5, 24), (20, 6), (1, 190))
SMALL_SHAPES = SHAPES[:7]                 # up to (2, 37): what the CPU emulation walks
SPLITS = {(5, 24): 2 * 24 * 24 + 7, (20, 6): 10 * 6 * 6 + 7}     # S2S_ET_MAX_PAIRS, as test_pair_kernels_tiled_layout_is_bit_identical sets it
EXPS = (5, 10, 15)
FAMILIES = ("flat", "trained-like", "offset-G", "offset-W", "small", "masked") + tuple(f"exp{e}" for e in EXPS)
ET = RN.TRUNK + "edge_transition_0."
IPA1 = RN.TRUNK + "ipa_1"
OUTPUTS = ("out", "proj")


def exp_of(family):
    return int(family[3:]) if family.startswith("exp") else 0


def capped(family):
    return family == "flat" or family.startswith("offset")


def tiles(B, N):
    """(pairs, 128-pair tiles, pairs in the last tile, 32-pair blocks, pairs in the last block)."""
    M = B * N * N
    return M, -(-M // 128), (M - 1) % 128 + 1, -(-M // 32), (M - 1) % 32 + 1


def _base_sd(family):
    sd = NC.trained_sd() if family == "trained-like" else synth_sd(0, 0.02)
    return {k: v.clone() for k, v in sd.items() if k.startswith(ET) or k.startswith(IPA1 + ".linear_b") or k.startswith(IPA1 + ".down_z")}


def _y_stats(sd, s, edge, parts=None):
    """(channel mean, channel std) [M] of the float64 y of every pair as the module's weights define it, and the largest hidden
    activation.  (From ``s`` the reference's G_j is centred, as the product's: the mean it leaves out is put back here.)"""
    tr = []
    RP.edge_transition(sd, ET, edge, s=s if parts is None else None, parts=parts, trace=tr)
    y = tr[-1]["pre_ln"]
    mean = y.mean(-1)
    if parts is None:
        B, N = edge.shape[:2]
        wf, bf = RN.lin(sd, ET + "final_layer")
        mean = mean + (tr[0]["out"] @ wf[:, 256:].double().t() + bf.double()).mean(-1)[RP.pair_index(B, N)[1]]
    return mean, y.std(-1, unbiased=False), max(float(tr[-3]["out"].abs().max()), float(tr[-1]["x"].abs().max()))


def offset_ratio(c, level):
    """[M]: |channel mean| / channel std of y, per pair of a case."""
    mean, sp, _ = _y_stats(c["sd"], c["s"], c["edge"], c["parts"] if level == "parts" else None)
    return mean.abs() / sp


def blocked(L, rows=4096):
    """``L`` applied to ``rows`` rows at a time (every row of a layer is its own computation: the same figures, out of the cache)."""
    def f(x, w, b=None, **kw):
        M, outs = x.shape[0], []
        for r0 in range(0, M, rows):
            sl = slice(r0, r0 + rows)
            kw2 = {k: (v[sl] if k in ("pre_scale", "pre_mask", "residual", "post_mask") and v is not None else v) for k, v in kw.items()}
            outs.append(L(x[sl], w, b[sl] if b is not None and b.dim() == 2 else b, **kw2))
        return torch.cat(outs)
    return f


@functools.lru_cache(maxsize=None)
def case(family, shape):
    """-> dict(family, B, N, sd, s [B, N, 256], edge [B, N, N, 128], mask [B, N] or None, exp, parts = (n' [B, N, 128], [A | B | G]
    [B, N, 896]) float32: the float64 per-node vectors of ``s`` rounded, with the family's operator-level plants).  Do not modify."""
    B, N = shape
    g = torch.Generator().manual_seed(90000 + 1000 * FAMILIES.index(family) + 7 * SHAPES.index(shape))
    sd = _base_sd(family)
    amp = NC.AMP_TRAINED if family == "trained-like" else 1.0
    s, edge, mask, exp = amp * torch.randn(B, N, 256, generator=g), amp * torch.randn(B, N, N, 128, generator=g), None, exp_of(family)
    if family == "small":
        s = s * NC.row_scales(B * N).view(B, N, 1)
        edge = edge * NC.row_scales(B * N * N).view(B, N, N, 1)
        for k in ("final_layer", "trunk.0", "trunk.2", "initial_embed"):     # (a bias would set the row's scale and hide the product)
            sd[ET + k + ".bias"].zero_()
    if family == "masked":
        mask = NC.mask_pattern(B * N, g, kind=SHAPES.index(shape) % 3).view(B, N)
        sd[ET + "trunk.2.bias"] = -sd[ET + "trunk.2.bias"].abs() - 1e-3
    if exp:
        # the first hidden layer x kw (as far as 32 kw w still packs into f16 with room to spare), the inputs x ki for the rest; the
        # other weights keep their ordinary size, so the fixed 2^5 weight packing keeps its precision
        target = 2.0 ** (13.5 + exp)
        w1, b1 = sd[ET + "trunk.0.weight"], sd[ET + "trunk.0.bias"]
        kw = min(target / _y_stats(sd, s, edge)[2], 2.0 ** 15.5 / (32.0 * float(w1.abs().max())))
        sd[ET + "trunk.0.weight"], sd[ET + "trunk.0.bias"] = w1 * kw, b1 * kw
        ki = 1.0
        n_p0 = RN.layer(s.reshape(B * N, 256), *RN.lin(sd, ET + "initial_embed"))
        cap = 2.0 ** 14 / max(float(edge.abs().max()), float(s.abs().max()), float(n_p0.abs().max()))
        for _ in range(4):       # (the biases do not follow the inputs: the hidden maximum is not quite linear in ki)
            ki = min(cap, ki * target / _y_stats(sd, ki * s, ki * edge)[2])
        s, edge = ki * s, ki * edge
    if family == "offset-W":
        mean0, sp, _ = _y_stats(sd, s, edge)
        tr = []
        RP.edge_transition(sd, ET, edge, s=s, trace=tr)
        x = tr[-1]["x"].clone()
        x[:, 256:] += tr[0]["out"][RP.pair_index(B, N)[1]]            # the whole final-layer input h2 + [e | n'_i | n'_j]
        v = torch.randn(384, generator=g).double()
        u = x @ v
        v = v * (2.0 * float(sp.median()) / float(u.std(unbiased=False).clamp_min(1e-30)) if B * N * N > 1 else 0.0)
        c = 24.0 * float(sp.median()) * (1.0 if float(torch.rand((), generator=g)) < 0.5 else -1.0)
        k = 1.0
        for _ in range(4):
            k *= 29.9 / float(((mean0 + k * (c + x @ v)).abs() / sp).max())
        sd[ET + "final_layer.weight"] = (sd[ET + "final_layer.weight"].double() + k * v[None, :]).float()
        sd[ET + "final_layer.bias"] = (sd[ET + "final_layer.bias"].double() + k * c).float()
    tr = []
    RN.edge_node_parts(sd, None, s.reshape(B * N, 256), trace=tr, prefix=ET)
    n_p = tr[0]["out"].float()
    ab = torch.cat([tr[1]["out"], tr[2]["out"], tr[3]["out"]], dim=-1).float()
    if family == "masked" and N > 1:
        ab[1::N, :384] = -1000.0           # residue 1 of every sample: A_i so negative that h1 = 0 for all its pairs; b2 < 0: h2 = 0
    parts0 = None
    if family == "offset-G":
        parts0 = (n_p.view(B, N, -1).contiguous(), ab.view(B, N, -1).clone())      # the per-node vectors in front of the plant
        parts = (n_p.view(B, N, -1), ab.view(B, N, -1))
        mean0, sp, _ = _y_stats(sd, None, edge, parts)
        mean0, sp = mean0.view(B, N, N), sp.view(B, N, N)
        room = (29.9 * sp - mean0.abs()).amin(1).clamp_min(0.0)      # [B, N] over i: what every pair of column j still takes
        cj = room * (0.7 + 0.3 * torch.rand(B, N, generator=g).double()) * torch.sign(torch.randn(B, N, generator=g).double())
        ab = ab.view(B, N, -1).clone()
        ab[..., 768:] = (ab[..., 768:].double() + cj[..., None]).float()
    return dict(family=family, B=B, N=N, sd=sd, s=s, edge=edge, mask=mask, exp=exp, parts0=parts0, parts=(n_p.view(B, N, -1).contiguous(), ab.view(B, N, -1).contiguous()))


LEVELS = ("parts", "module")


def levels(family):
    """offset-G exists at the operator level only; offset-W at the module level (its per-node vectors are the reference's, whose G_j
    is centred: they carry the part of the offset that W_f[:, :256] leaves, which is not the family's condition)."""
    return ("parts",) if family == "offset-G" else (("module",) if family == "offset-W" else LEVELS)


def run(c, level, dtype=torch.float64, L=RN.layer, L_hidden=None, device="cpu", wrong=None, rows=8192):
    """``ref_pair.edge_transition`` + the projection of a case at a contract level -> (out rows [M, 128], projection rows [M, 40], trace
    with the projection's record last).  On ``device`` the pair rows are evaluated ``rows`` samples' worth at a time (whole samples)."""
    B, N = c["B"], c["N"]
    to = lambda t: None if t is None else t.to(device)  # noqa: E731
    sd = {k: v.to(device) for k, v in c["sd"].items()}
    per = max(1, rows // (N * N))
    outs, projs, traces = [], [], []
    for b0 in range(0, B, per):
        sl = slice(b0, min(B, b0 + per))
        tr = [] if dtype == torch.float64 else None          # (the float32 chain: no trace, the layers in row blocks)
        if tr is None and L is RN.layer:
            L = blocked(RN.layer)
        kw = dict(s=to(c["s"][sl])) if level == "module" else dict(parts=tuple(to(t[sl]) for t in c["parts"]))
        mask = to(c["mask"][sl]) if c["mask"] is not None else None
        out = RP.edge_transition(sd, ET, to(c["edge"][sl]), mask, dtype=dtype, L=L, L_hidden=L_hidden, trace=tr, exp=c["exp"], wrong=wrong, **kw)
        unmasked = None
        if wrong == "projection_of_unmasked_row":
            unmasked = RP.edge_transition(sd, ET, to(c["edge"][sl]), None, dtype=dtype, L=L, L_hidden=L_hidden, exp=c["exp"], **kw)
        if tr is None:
            pr, prec = RP.projection(sd, IPA1, out, None, dtype=dtype, wrong=wrong, unmasked=unmasked), None
        elif L is RN.layer and L_hidden is None:
            pr, prec = RP.projection(sd, IPA1, out, tr[-1], dtype=dtype, wrong=wrong, unmasked=unmasked)
        else:      # the plane emulation: the projection stage through the same layer function
            w = torch.cat([sd[IPA1 + ".linear_b.weight"], sd[IPA1 + ".down_z.weight"]])
            b = torch.cat([sd[IPA1 + ".linear_b.bias"], sd[IPA1 + ".down_z.bias"]])
            pr = L(out.reshape(-1, 128), w, b, dtype=dtype)
            prec = None
        recs = (tr or []) + ([prec] if prec is not None else [])
        for rec in recs:
            rec["level"] = level          # (``level_of``: which r16 the bound of these pairs takes)
        outs.append(out.reshape(-1, 128)); projs.append(pr); traces.append(recs)
    return torch.cat(outs), torch.cat(projs), traces


@functools.lru_cache(maxsize=None)
def ref(family, shape, level):
    """The float64 evaluation on the CPU.  Shared; do not modify."""
    return run(case(family, shape), level)


# ---------------------------------------------------------------------------------------------------- the planes, emulated
STAGES = ("n'", "A", "B", "G", "layer1", "layer2", "final", "projection")      # the layers of a module-level evaluation, in call order


def stages(level):
    """The layers of an evaluation at ``level``: the per-node layers exist at the module level only."""
    return STAGES if level == "module" else STAGES[4:]


def level_of(traces):
    """The contract level the float64 traces of ``run`` were taken at, as ``run`` stamped it on their records."""
    found = {rec["level"] for tr in traces for rec in tr}
    assert len(found) == 1 and found <= set(LEVELS), found
    return found.pop()


def emulation(c, level, flags=(), stage=None):
    """Keyword arguments of ``run`` for the CPU emulation of the f16 planes on a case: ``ref_node.f16x3_layer``, the layers that read
    hidden activations on 2^-exp x their input under a block exponent, the projection through the same layer function.  ``flags``
    (drop_xl | drop_wl | flush_subnormals of ``ref_node.split_f16x3``: planted mistakes) apply to every layer, or with ``stage`` (a
    name of ``stages(level)``) to that layer alone: the layer functions count their calls, one evaluation being len(stages) of them."""
    kw = {k: True for k in flags}
    pick = lambda **f: (RN.f16x3_layer(**f), RP.scaled_planes_layer(c["exp"], **f) if c["exp"] else None)  # noqa: E731
    if stage is None:
        return dict(zip(("L", "L_hidden"), pick(**kw)))
    names, calls = stages(level), [0]
    k = names.index(stage)
    (L0, H0), (L1, H1) = pick(), pick(**kw)

    def counted(plain, wrong):
        def f(*a, **kwargs):
            i, calls[0] = calls[0] % len(names), calls[0] + 1
            return (wrong if i == k else plain)(*a, **kwargs)
        return f
    return dict(L=counted(L0, L1), L_hidden=counted(H0, H1) if c["exp"] else None)


@functools.lru_cache(maxsize=None)
def emulated(family, shape, level):
    """(out rows, projection rows) of the faithful emulation on a case of SMALL_SHAPES.  Shared; do not modify."""
    c = case(family, shape)
    return run(c, level, **emulation(c, level))[:2]


# ---------------------------------------------------------------------------------------------------- the measure
def out_scale(rec):
    """[M]: max_c |out64 - beta| m: the normalised row without the LayerNorm's shift (0 on masked pairs)."""
    beta = rec["ln"][1].to(rec["out"])
    m = 1.0 if rec["post_mask"] is None else rec["post_mask"][:, None]
    return ((rec["out"] - beta * m).abs()).amax(-1)


def masked_rows(rec):
    M = rec["out"].shape[0]
    return torch.zeros(M, dtype=torch.bool, device=rec["out"].device) if rec["post_mask"] is None else rec["post_mask"] == 0


def errors(got, traces, output):
    """-> (errors [M] (nan on masked pairs), exact [M] bool: masked pairs on which ``got`` equals the reference bit for bit,
    masked [M] bool) of ``got`` rows against the float64 traces of ``run``."""
    errs, exact, masked, r0 = [], [], [], 0
    for tr in traces:
        rec_out, rec = tr[-2], tr[-1 if output == "proj" else -2]
        M = rec["out"].shape[0]
        gd = got[r0:r0 + M].to(rec["out"].device).double()
        scale = NC.record_scale(rec) if output == "proj" else out_scale(rec)
        dead = masked_rows(rec_out)
        e = (gd - rec["out"]).abs().amax(-1) / scale.clamp_min(1e-300)
        errs.append(torch.where(dead | (scale == 0), torch.full_like(e, float("nan")), e))
        exact.append((gd == rec["out"]).all(-1))
        masked.append(dead)
        r0 += M
    return torch.cat(errs), torch.cat(exact), torch.cat(masked)


def floor(traces, output):
    """[M]: F of every pair (node_cases.floors through the whole trace, over the pair's scale)."""
    out = []
    for tr in traces:
        i = len(tr) - 1 if output == "proj" else len(tr) - 2
        f = NC.floors(tr)[i].amax(-1)
        scale = NC.record_scale(tr[i]) if output == "proj" else out_scale(tr[i])
        out.append(torch.where(scale > 0, f / scale.clamp_min(1e-300), torch.zeros_like(f)))
    return torch.cat(out)


@functools.lru_cache(maxsize=None)
def d32(family, level):
    """{output: D32} of a (family, level): ref_pair in float32 against float64, pooled over SHAPES."""
    worst = {o: 0.0 for o in OUTPUTS}
    for shape in SHAPES:
        out32, proj32, _ = run(case(family, shape), level, dtype=torch.float32)
        _, _, traces = ref(family, shape, level)
        for o, got in (("out", out32), ("proj", proj32)):
            worst[o] = max(worst[o], NC.nanmax(errors(got, traces, o)[0]))
    return worst


@functools.lru_cache(maxsize=None)
def r16(family, level):
    """{output: r16} of a (family, level): the largest error / F_pair of the faithful plane emulation against float64 over every
    valid pair with F_pair > 0 of SMALL_SHAPES -- the share of the a-priori floor that the format uses."""
    worst = {o: 0.0 for o in OUTPUTS}
    for shape in SMALL_SHAPES:
        traces = ref(family, shape, level)[2]
        for o, got in zip(OUTPUTS, emulated(family, shape, level)):
            e, f = errors(got, traces, o)[0], floor(traces, o)
            ok = ~torch.isnan(e) & (f > 0)
            if ok.any():
                worst[o] = max(worst[o], float((e[ok] / f[ok]).max()))
    return worst


def floor_share(family, level, output):
    """min(1, 3 x r16): the factor on F_pair in the bound of arith "f16x3"."""
    return min(1.0, 3.0 * r16(family, level)[output])


def judged(got, traces, output, family, d, arith="f16x3", rule="measured"):
    """``got`` rows against the float64 traces under the bound rule -> dict(achieved, bound, pair: the pair with the largest error /
    bound; exact: masked pairs all exact; largest, largest_bound: the largest error of any pair against base + share x the largest F).
    ``rule`` "a-priori" judges with the whole F (share 1): the rule before r16, kept to show what it let through."""
    e, exact, masked = errors(got, traces, output)
    base = min(3.0 * d, NC.CAP) if capped(family) else 3.0 * d
    b, fmax = torch.full_like(e, base), 0.0
    if arith == "f16x3":
        share = 1.0 if rule == "a-priori" else floor_share(family, level_of(traces), output)
        f = share * floor(traces, output).to(e)
        b, fmax = b + f, float(f.max()) if f.numel() else 0.0
    ratio = torch.where(torch.isnan(e), torch.zeros_like(e), e / b)
    r = int(ratio.argmax()) if ratio.numel() else 0
    return dict(achieved=0.0 if torch.isnan(e[r]) else float(e[r]), bound=float(b[r]), pair=r, exact=bool(exact[masked].all()),
                largest=NC.nanmax(e), largest_bound=base + fmax)


def check(got, traces, output, family, d, arith="f16x3"):
    """-> (achieved, bound, worst pair, masked pairs all exact) of ``got`` rows: the pair with the largest error / bound, the bound of
    a pair being 3 x D32 (capped for flat and offset) + min(1, 3 x r16) x its F (f16x3 only)."""
    j = judged(got, traces, output, family, d, arith)
    return j["achieved"], j["bound"], j["pair"], j["exact"]


# ---------------------------------------------------------------------------------------------------- the edge embedding's last layer
EMB_SHAPES = ((3, 7), (1, 33))            # one below 32 residues, one from 32


@functools.lru_cache(maxsize=None)
def embed_offset_case(shape):
    """The embedder's inputs at ``shape`` and a state dict whose last pair-MLP layer (edge_embed.4) carries a common component
    c + v^T h in bias and rows, scaled so that every pair's |channel mean| / channel std of the value in front of the LayerNorm is at
    most 30 (and at least 20 for a tenth of the pairs).  -> dict(sd, residue_idx, t, fixed_mask, ca, ratio [B N N])."""
    import embed_cases as EC
    import ref_embed as RE
    import torch.nn.functional as F

    B, N = shape
    g = torch.Generator().manual_seed(95000 + N)
    sd = {k: v.clone() for k, v in synth_sd(0, 0.02).items() if k.startswith("embedder.")}
    idx = torch.arange(N)[None].repeat(B, 1)
    t = torch.tensor([EC.T_VALUES[b % len(EC.T_VALUES)] for b in range(B)])
    fixed = (torch.rand(B, N, generator=g) > 0.6).float()
    ca, _ = EC.clear_of_bin_edges(8.0 * torch.randn(B, N, 3, generator=g), g)
    _, pair32 = RE.features32(idx, t, fixed, ca)
    p = "embedder.edge_embed."
    h = pair32.reshape(-1, pair32.shape[-1]).double()
    h1 = F.relu(F.linear(h, sd[p + "0.weight"].double(), sd[p + "0.bias"].double()))
    h = F.relu(F.linear(h1, sd[p + "2.weight"].double(), sd[p + "2.bias"].double()))

    def stats(w, b):
        y = F.linear(h, w, b)
        return y.mean(-1), y.std(-1, unbiased=False)

    w4, b4 = sd[p + "4.weight"].double(), sd[p + "4.bias"].double()
    mean0, sp = stats(w4, b4)
    v = torch.randn(h.shape[1], generator=g).double()
    u = h @ v
    v = v * 2.0 * float(sp.median()) / float(u.std(unbiased=False).clamp_min(1e-30))
    c, k = 24.0 * float(sp.median()), 1.0
    for _ in range(4):
        k *= 29.9 / float(((mean0 + k * (c + h @ v)).abs() / sp).max())
    sd[p + "4.weight"], sd[p + "4.bias"] = (w4 + k * v[None, :]).float(), (b4 + k * c).float()
    mean1, sp1 = stats(sd[p + "4.weight"].double(), sd[p + "4.bias"].double())
    return dict(sd=sd, B=B, N=N, residue_idx=idx, t=t, fixed_mask=fixed, ca=ca, ratio=mean1.abs() / sp1, h1=h1)


def embed_floor(c):
    """[B N N]: F of the edge embedding's output per pair: its two 128 x 128 layers read planes (the first layer is a sum of
    gathered float32 rows), so the floor is that of the chain relu(W2 h1 + b2) -> LayerNorm(W3 . + b3) on the float64 h1."""
    tr = _embed_chain(c)
    f, scale = NC.floors(tr)[-1].amax(-1), out_scale(tr[-1])
    return torch.where(scale > 0, f / scale.clamp_min(1e-300), torch.zeros_like(f))


def _embed_chain(c, L=RN.layer):
    p, sd, tr = "embedder.edge_embed.", c["sd"], []
    h2 = L(c["h1"], sd[p + "2.weight"], sd[p + "2.bias"], relu=True, trace=tr)
    L(h2, sd[p + "4.weight"], sd[p + "4.bias"], ln=RN.ln_of(sd, p + "5"), trace=tr)
    return tr


@functools.lru_cache(maxsize=None)
def embed_r16():
    """r16 of the edge embedding's chain: the plane emulation of its two layers against float64 on the float64 h1, error / F per pair,
    the largest over EMB_SHAPES.  The bound of a pair is 3 x D32 (capped) + min(1, 3 x r16) x F_pair, as for the EdgeTransition."""
    worst = 0.0
    for shape in EMB_SHAPES:
        c = embed_offset_case(shape)
        rec, got = _embed_chain(c)[-1], _embed_chain(c, RN.f16x3_layer())[-1]["out"]
        e, f = (got - rec["out"]).abs().amax(-1) / out_scale(rec).clamp_min(1e-300), embed_floor(c)
        ok = (out_scale(rec) > 0) & (f > 0)
        if ok.any():
            worst = max(worst, float((e[ok] / f[ok]).max()))
    return worst
