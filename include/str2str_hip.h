/* str2str_hip.h — C ABI of libstr2str_hip.so (MI355X / gfx950 kernels for the Str2Str sampling path).
 *
 * Drop-in boundary: the reference has no FFI layer — its seams are Python call
 * sites.  Each entry point below replaces the chain of eager PyTorch ops behind ONE such call site
 * (cited per function as reference file:line) and is what a binding for that call site would load:
 * plain device pointers, sizes and a HIP stream; no torch types.  INTEGRATION.md shows the ctypes
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller (in this repo: torch tensors); kernels never
 *     allocate, free or synchronise; outputs must be pre-allocated, contiguous, 16-byte aligned;
 *   - `stream` is a hipStream_t (0 = default stream); work is only enqueued;
 *   - float = IEEE binary32; frames are "tensor_7": quaternion (w,x,y,z) + translation (x,y,z)
 *     (Rigid.to_tensor_7, src/common/rigid_utils.py:1203-1215);
 *   - return value: 0 on success, otherwise a hipError_t (argument errors = hipErrorInvalidValue);
 *   - re-entrant across streams and threads: every call takes what it reads and writes as arguments (the range guard's buffer
 *     included, `range_words` below); the only library state is the backbone table, uploaded per device.
 */
#ifndef STR2STR_HIP_H
#define STR2STR_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* Library ABI version (bumped on any signature change).  Still 40 with s2s_backbone_sasa and s2s_ca_scattering: entry points were added, no
 * signature changed. */
int s2s_abi_version(void);

/* Arithmetic.  Every matrix product of the path exists in two forms behind the same operator contract:
 *   "f16x3" (default): operands split into f16 pairs, three products per block on the 16-bit matrix cores, fp32 accumulation --
 *           fp32-equivalent in precision, but an activation must stay below f16's 65504;
 *   "f32":  exact fp32 MFMA, no range limit (s2s_edge_transition, s2s_edge_embed, s2s_ipa_attention, s2s_node_linear_f32,
 *           s2s_encoder_attention): the reference arithmetic and the automatic fallback.
 * Range guard: every entry point that splits values into f16 planes takes `int* range_words`, an 8-int DEVICE buffer passed per call
 * (NULL disables the reports).  Its kernels keep a running maximum of the values they split and OR a bit into word 0 when that
 * maximum reaches 2^15 or is not finite (bits: 1 node GEMM, 2 pack_planes, 4 edge transition, 8 edge embedding, 16 IPA points,
 * 32 encoder attention).  Word 1 + log2(bit) collects magnitude buckets of the same family: bit e set = a launch saw a maximum in
 * [2^(8+e), 2^(9+e)) (e = 8: 2^16 or more); nothing is written below 2^8.  The caller clears / reads the buffer (no kernel waits for
 * it) and decides what a raised bit means: str2str_amd/sampler.py re-runs the chunk with ONLY the flagged kernel families on their
 * exact fp32 kernels. */

/* ---- Pair-stream MLPs (fp32 MFMA).  Weight blobs are "packed" for the kernels' lane order:
 *      packed[((s4*T + t)*64 + lane)*4 + q] = W[32*t + (lane & 31)][8*s4 + 4*(lane >> 5) + q]
 *      for W [32*T, 8*S4] row-major (str2str_amd/ops/packing.py: pack_weight does this).  s2s_edge_transition takes the
 *      TILE-MAJOR order instead: packed[((t*S4 + s4)*64 + lane)*4 + q] (pack_weight(..., tile_major=True)). ---- */

/* EdgeTransition.forward (src/models/net/layers.py:170-185) followed by the edge-mask multiply of
 * TranslationIPA.forward (src/models/net/ipa.py:371-372).
 *   edge     [B,N,N,128]  in        node_ab [B,N,768] = [W1[:,128:256].n'+b1 | W1[:,256:384].n']
 *   node_p   [B,N,128]    n' = initial_embed(node)
 *   w1_packed: W1[:, :128] (384x128); w2_packed: W2 (384x384); wf_packed: final_layer.weight (128x384)
 *   b2 [384], bf [128], ln_gamma/ln_beta [128], mask [B,N] or NULL, out [B,N,N,128] (may not alias edge).
 *   Optional fused epilogue (proj_w_packed != NULL): the NEXT IPA block's linear_b/down_z (see s2s_pair_project)
 *   applied to the freshly produced pair vectors while they are still in registers -> proj_attn_bias, proj_pair_z. */
int s2s_edge_transition(const float* edge, const float* node_ab, const float* node_p, const float* w1_packed,
                        const float* w2_packed, const float* wf_packed, const float* b2, const float* bf,
                        const float* ln_gamma, const float* ln_beta, const float* mask, float* out, int n_samples,
                        int n_res, float ln_eps, const float* proj_w_packed, const float* proj_bias_cat64,
                        float* proj_attn_bias, float* proj_pair_z, void* stream);

/* The same operator on split-f16 MFMA ("f16x3", csrc/edge_transition_f16.h; the default): every fp32 operand as two f16 numbers (11 + 11
 * bits + the residue's sign = fp32's 24), products w_h x_h + w_h x_l + w_l x_h with the weights stored as the split of 2^5 w (2^-5
 * back in the epilogues), fp32 accumulation -- three matrix instructions per block, the dropped w_l x_l below one fp32 rounding.
 * Activations must stay below f16's 65504 (range guard above).  weight_stream: 30 (+1 with the fused projection) stages x 32 KiB
 * of f16 A fragments (W_h, W_l) in slot order (ops.pack_f16x3_stream, ops.pack_f16x2_layer for the projection stage; the order is
 * part of the ABI version).
 *   Optional fused epilogue (proj_attn_bias != NULL): the NEXT IPA block's linear_b / down_z (see s2s_pair_project);
 *   the stream then carries a 31st stage with the chain-packed 64x128 [linear_b; down_z; 0] matrix, proj_bias_cat64 [64];
 *   outputs proj_attn_bias [B,8,N,N] (head-major) and proj_pair_z [B,N,N,32].
 *   Pair-tensor layouts (io_layout; 0 = the reference's [B,N,N,128] on both sides).  Between the library's own pair kernels the tensor
 *   may travel TILED: the flat pair sequence in blocks of 32 pairs (16 KiB), block b = pairs 32 b .. 32 b + 31, inside a block
 *   [16 groups g][2 halves h][32 pairs n][4 floats] = channels 8 g + 4 h .. + 3 of pair 32 b + n at float offset 4096 b + 256 g + 128 h + 4 n
 *   -- the order in which a wavefront's lanes hold a 32-pair tile, so that one load / store instruction covers 8 whole cache lines
 *   instead of 32 B in each of 32 (ops.pair_tiled / ops.pair_untiled convert).  The buffer of a tiled tensor holds whole blocks
 *   (B N N rounded up to 32 pairs; the padding is never read as data).
 *     io_layout bit 0: edge is tiled;  bit 1: out is written tiled;  bit 2: out is not written at all (out may be NULL; needs the
 *     fused projection -- the last EdgeTransition of the trunk, whose pair vectors only feed the next block's projections).
 *   BY CLASS (the first EdgeTransition behind the edge embedding's class path, below).  The embedding's pair tensor need not exist: every
 *   row of it is a copy of a record of the class table.  edge is then ONE buffer of 4-byte words,
 *     [ M32 int32: the class row of every pair in flat pair order, -1 where m_i m_j = 0 | a record of zeros | the class table's records ],
 *   M32 = n_samples n_res^2 rounded up to 32 (the records start 16-byte aligned; both offsets follow from n_samples and n_res), as
 *   s2s_edge_embed_classes_f16x3 (table = edge + M32 + one record) and s2s_edge_embed_expand (out = edge, out_tiled = 2) fill it; the
 *   zero record is the caller's (ops.edge_embed_classes_f16x3 zeroes it).  Rows are addressed by 32-bit BYTE offsets: the records
 *   (zero record + table) must stay below 4 GB -- the row count is not an argument here, so the caller answers for it (the class
 *   path's eligibility rule, ops.edge_embed_classes_eligible, refuses larger tables).  A
 *   lane reads the z[128] of record index + 1 -- 16-byte groups at a stride of 8 floats, as of a row-major row -- so a masked pair
 *   reads zeros: z x (m_i m_j) for a 0/1 mask.  The index words past the last pair are never read.
 *     io_layout bit 3: edge is such a buffer (not with bit 0; needs the fused projection, else hipErrorInvalidValue);
 *     bit 4 (with bit 3 only): its records are 168 floats (the table was built with the fused projection), else 128.
 *   A split launch (S2S_ET_MAX_PAIRS) moves the index pointer by whole samples; the records stay where they are.
 *   node_ab HERE is [B,N,896] = [ 2^-e (W1[:,128:256].n' + b1) | 2^5 W1[:,256:384].n' | 2^(5-e) (Wf[:,256:384].n' + bf) ]  (e = prescale_exp
 *   below; W1 = the first hidden layer, Wf / bf = final_layer): everything the pair (i, j) takes from its two NODES through a linear
 *   layer, computed once per node.  The column half B_j (384) is the START VALUE of the layer-1 accumulators, which carry 2^5 x the
 *   layer output, and is loaded straight into them; the row half A_i (384) is added in the epilogue at the planes' scale; the third
 *   group G_j (128) is the start value of the FINAL layer's accumulators: the layer reads x = h2 + [e | n'_i | n'_j]
 *   (layers.py:181), and the part of it that depends on node j alone, Wf[:,256:384].n'_j + bf, does not have to be added to the
 *   hidden values of every pair.  (The i-side residual n'_i is still added in the kernel: node_p [B,N,128] = n'.)  All factors are
 *   powers of two: the caller folds them into the per-node layers that produce node_ab (EdgeTransition.ab16_specs) or scales a plain
 *   node_ab (ops.edge_transition_f16x3 does, unless told that node_ab has this form already).
 *   CENTRED FINAL LAYER.  LayerNorm(Wf x + bf) = LayerNorm(C Wf x + C bf) exactly for C = I - 1 1^T / 128, so the kernel is handed
 *   the final layer without the component common to its 128 output channels: the Wf stages of weight_stream are packed from C Wf
 *   and G_j is C (Wf[:,256:384].n'_j + bf) -- both centred in float64 on the host where they are packed (EdgeTransition._packed,
 *   .node_layers; ops.edge_transition_f16x3 centres a plain node_ab's third group).  y then has channel mean 0 up to rounding for
 *   every pair: the LayerNorm's plain mean has nothing to lose, and the accumulators that start at 2^5 G_j round at the spread's
 *   magnitude, not at an offset's (a trained checkpoint's common component is unconstrained: the loss has no gradient on it).  The
 *   kernel itself does not depend on it -- uncentred operands give the same function with an error that grows with
 *   |channel mean| / channel spread (measured at 30: 1.9e-5 of the row's scale through the start value, 2.6e-5 through the fp32
 *   kernel's mean).  The same holds for s2s_edge_transition (wf_packed, bf centred: EdgeTransition._packed_f32, ._bf_centred) and
 *   for the last layer of both edge-embedding kernels (w3_packed / the W3 stages and b3: EmbeddingModule._weights). */
int s2s_edge_transition_f16x3(const float* edge, const float* node_ab, const float* node_p, const void* weight_stream,
                              const float* b2, const float* ln_gamma, const float* ln_beta,
                              const float* mask, float* out, int n_samples, int n_res, float ln_eps, int io_layout,
                              const float* proj_bias_cat64, float* proj_attn_bias, float* proj_pair_z, int prescale_exp,
                              int* range_words, void* stream);
/*   prescale_exp = e in 0 .. 15 (0: none): BLOCK EXPONENT of the hidden activations.  The two hidden layers' outputs (relu(layer 1),
 *   relu(layer 2) + x) are kept as f16 planes of 2^-e x their value: relu is positively homogeneous, so the factor rides in
 *   constants the epilogues apply anyway and LayerNorm removes it -- exact for a power of two, no extra instruction, e = 0 is bit
 *   for bit the unscaled kernel.  The row half and the third group of node_ab must then be handed in multiplied by 2^-e (see above).
 *   It moves the kernel's usable range from 2^15 to 2^(15+e) at the price of f16's subnormal spacing on activations below
 *   2^(e-3) (absolute error 2^(e-25): far below the large activations' own rounding); the range guard sees the SCALED values. */

/* EmbeddingModule.forward, edge branch (src/models/net/denoising_ipa.py:137-158, calc_distogram
 * src/common/geo_utils.py:44-56) + edge-mask multiply (denoising_ipa.py:187).
 *   node_a/node_b [B,N,128]: row / column parts of the first Linear (incl. bias in node_a)
 *   rel_table [n_rel,128]: first-layer image of posemb(d), d = idx_i - idx_j, row d + rel_offset
 *   bin_table [n_bins,128]: first-layer columns of the distogram one-hot; bin_lower [n_bins]
 *   residue_idx [B,N] int64; ca_xyz [B,N,3] (self-conditioning CA, Angstrom)
 *   w2/w3 packed 128x128; b2,b3,ln_gamma,ln_beta [128]; out [B,N,N,128]; proj_*: optional fused pair projection as above. */
int s2s_edge_embed(const float* node_a, const float* node_b, const float* rel_table, const float* bin_table,
                   const float* bin_lower, const long long* residue_idx, const float* ca_xyz, const float* w2_packed,
                   const float* w3_packed, const float* b2, const float* b3, const float* ln_gamma, const float* ln_beta,
                   const float* mask, float* out, int n_samples, int n_res, int rel_offset, int n_rel, int n_bins,
                   float ln_eps, const float* proj_w_packed, const float* proj_bias_cat64, float* proj_attn_bias,
                   float* proj_pair_z, void* stream);

/* The edge embedding on split-f16 MFMA (see s2s_edge_transition_f16x3; the default).  weight_stream: 4 stages x 32 KiB (W2 | W3,
 * chain-packed (W_h, W_l) fragments in slot order: ops.pack_f16x3_embed_stream) + a 5th stage with the [linear_b; down_z; 0]
 * matrix when the fused projection is requested (proj_attn_bias != NULL).
 *   Layout difference to s2s_edge_embed: node_b, rel_table and bin_table are COLUMN-BLOCKED --
 *   node_b [B][32][N][4], rel_table [32][n_rel][4], bin_table [32][n_bins][4], element [c][row][q] = channel 4c + q of that row
 *   (ops.column_blocked) -- so that the gathers of neighbouring pairs share cache lines; node_a stays [B,N,128];
 *   bin_lower must ascend (torch.linspace), n_bins <= 32.  Pair indices are 32-bit inside a launch: the entry point splits the
 *   samples over several launches when B*N*N >= 2^31 (N*N itself and n_rel*512 must stay below 2^31 / 2^32).
 *   out_tiled = 1: out is written in the tiled pair layout (s2s_edge_transition_f16x3), its buffer holds whole 32-pair blocks. */
int s2s_edge_embed_f16x3(const float* node_a, const float* node_b, const float* rel_table, const float* bin_table,
                         const float* bin_lower, const long long* residue_idx, const float* ca_xyz,
                         const void* weight_stream, const float* b2, const float* b3, const float* ln_gamma,
                         const float* ln_beta, const float* mask, float* out, int n_samples, int n_res, int rel_offset,
                         int n_rel, int n_bins, float ln_eps, int out_tiled, const float* proj_bias_cat64,
                         float* proj_attn_bias, float* proj_pair_z, int* range_words, void* stream);

/* The edge embedding by CLASS, for chunks that share one timestep (replicas of a target: every sampler call).  node_a[b,i] is then
 * one row per value of fixed_mask[b,i] and node_b[b,j] likewise, so with a 0/1 fixed mask a pair's first-layer sum -- and z,
 * attn_bias and pair_z before the edge mask -- depends only on its class (fa, fb, d, bin): fa / fb the class of the fixed mask at
 * i / j, d the row of rel_table (idx_i - idx_j + rel_offset, clamped), bin the distogram bin or -1 for none.  Two launches:
 *
 * s2s_edge_embed_classes_f16x3 runs the kernel body of s2s_edge_embed_f16x3 (same slots, split, LayerNorm, projection) once per row
 *   r = ((fa * 2 + fb) * n_rel + d) * (n_bins + 1) + (bin + 1)
 * of the table: (n_fixed == 2 ? 4 : 1) * n_rel * (n_bins + 1) records, row-major, of 168 floats z[128] | attn_bias[8] | pair_z[32]
 * with the fused projection (proj_bias_cat64 != NULL; weight_stream then has its 5th stage), else of 128 floats (z).
 *   node_a2 [n_fixed,128], node_b2 column-blocked [32][n_fixed][4]: the operands s2s_embed_assemble gives for a pseudo-sample of
 *   n_fixed residues whose fixed mask runs over the values present (the same expression as for the chunk: the same floats);
 *   rel_table / bin_table column-blocked as above.  The first-layer sum keeps the association ((a + b) + r) + kb * k, the edge mask
 *   is 1.  The range report covers every row of the table -- a superset of the rows in use, so the guard can only fire earlier.
 *
 * s2s_edge_embed_expand computes every pair's class with the edge embedding's own device functions (csrc/edge_embed_class.h) and
 * writes out = z[row] * (m_i m_j) (row-major or tiled, as above), attn_bias [B,8,N,N] and pair_z [B,N,N,32] (both optional, together)
 * = the row's, or proj_bias_cat64 where m_i m_j = 0.  fixed_cls [B,N] int32: index of fixed_mask[b,i] among the n_fixed values.
 * Bit for bit s2s_edge_embed_f16x3's outputs where the edge mask is non-zero (and equal as numbers where it is zero) under the
 * ELIGIBILITY rules, which are the caller's: one timestep row for the whole chunk, fixed mask exactly 0/1, node mask exactly 0/1
 * (or NULL).  It pays when the table is small against B*N*N (EmbeddingModule.embed).  Launch split and S2S_EE_MAX_PAIRS as above.
 *   out_tiled = 2 (INDEX MODE): z is not written.  out receives one int32 per pair in flat pair order -- the pair's class row, or -1
 *   where m_i m_j = 0: the index words of the by-class buffer of s2s_edge_transition_f16x3 (io_layout bit 3), whose zero record is the
 *   caller's to provide.  attn_bias and pair_z as in the other modes.
 *   Records are 168 floats whenever proj_bias_cat64 != NULL -- also with proj_attn_bias = proj_pair_z = NULL, which expands z alone out
 *   of a table that was built with the fused projection -- else 128. */
int s2s_edge_embed_classes_f16x3(const float* node_a2, const float* node_b2, const float* rel_table, const float* bin_table,
                                 const void* weight_stream, const float* b2, const float* b3, const float* ln_gamma,
                                 const float* ln_beta, float* table, int n_fixed, int n_rel, int n_bins, float ln_eps,
                                 const float* proj_bias_cat64, int* range_words, void* stream);
int s2s_edge_embed_expand(const float* table, const int* fixed_cls, const float* bin_lower, const long long* residue_idx,
                          const float* ca_xyz, const float* mask, const float* proj_bias_cat64, float* out, int out_tiled,
                          float* proj_attn_bias, float* proj_pair_z, int n_samples, int n_res, int rel_offset, int n_rel,
                          int n_bins, void* stream);

/* linear_b and down_z of InvariantPointAttention (src/models/net/ipa.py:177, :253) in one pass over z.
 *   w_packed: [linear_b.weight (8 rows); down_z.weight (32 rows); 24 zero rows] (64x128) packed
 *   bias_cat64 [64]; attn_bias [B,8,N,N] (head-major: what s2s_ipa_attention streams per head); pair_z [B,N,N,32]. */
int s2s_pair_project(const float* edge, const float* w_packed, const float* bias_cat64, float* attn_bias, float* pair_z,
                     int n_samples, int n_res, void* stream);

/* ---- Invariant point attention ---- */

/* Point generation: split/stack of the coordinate-major linear outputs and Rigid.apply
 * (src/models/net/ipa.py:144-171; src/common/rigid_utils.py:1107-1120).
 *   rigids7 [M,7] (translation already x coordinate_scaling), q_pts_lin [M,3*H*Pq], kv_pts_lin [M,3*H*(Pq+Pv)]
 *   q_pts,k_pts [M,H,Pq*3]; v_pts [M,H,v_pts_stride] as (x,y,z,0) per point, zero padded (stride 64). */
int s2s_ipa_prep_points(const float* rigids7, const float* q_pts_lin, const float* kv_pts_lin, float* q_pts, float* k_pts,
                        float* v_pts, long long n_frames, int n_heads, int n_qk_points, int n_v_points, int v_pts_stride,
                        void* stream);

/* Attention core of InvariantPointAttention.forward (src/models/net/ipa.py:183-252): logits
 * (scalar + pair bias + point distances + mask), softmax over keys, o / o_pt (inverse-transformed,
 * with norms), written in linear_out's concat order (ipa.py:259-266):
 *   out [B,N, H*C | H*Pv (x) | H*Pv (y) | H*Pv (z) | H*Pv (norm) | H*c_pair_z]   (the o_pair columns are left to
 *   s2s_ipa_opair).
 *   q [B,N,H,C]; kv [B,N,H,2C]; attn_bias [B,H,N,N]; head_w_scaled [H] = softplus(head_weights)*sqrt(1/(3*(Pq*9/2))).
 *   logits_out [B,H,N,N] (masked logits; may alias attn_bias), stats_out [B,H,N,2] (row maximum, sum of exp).
 * Supported shape: C=256, Pq=8, Pv=12, c_pair_z=32, H multiple of 4 (configs/model/diffusion.yaml:29-40). */
int s2s_ipa_attention(const float* q, const float* kv, const float* q_pts, const float* k_pts, const float* v_pts64,
                      const float* attn_bias, float* logits_out, float* stats_out, const float* mask, const float* rigids7,
                      const float* head_w_scaled, float* out, int n_samples, int n_res, int n_heads, int c_hidden,
                      int n_qk_points, int n_v_points, int c_pair_z, float inf, float eps, void* stream);

/* The DEFAULT attention core (csrc/ipa_attention_f16w.hip), on operands that are ALREADY split into f16 pairs (x_h, x_l) in MFMA
 * fragment order: q_xp / k_xp = packed planes [rows/32][16 H][2][64][8] of the q and k projections (out_xp of s2s_node_linear with
 * linear_q and the k rows of linear_kv), v_vf = s2s_node_linear_vfrag of the v rows of linear_kv.
 * s2s_ipa_prep_points_f16 (ipa.py:144-171) writes the global-frame points as fragments: qp_xp [rows/32][H][2][2][64][8] (query
 * points x head_w_scaled[h] / sqrt(1/(3 c_hidden))), kp_xp (key points), vp_vf [rows/32][H][2][2][2][64][8] (value points as
 * (x,y,z,0) groups), and q2 / k2 [rows/32][H][32] = -1/2 head_w_scaled[h] |points|^2: the point term of the logits (ipa.py:191-205)
 * is evaluated as  w q.k - w/2 |q|^2 - w/2 |k|^2  with the cross term on the matrix cores.
 * s2s_ipa_attention_f16w: three products per block (a_h b_h + a_h b_l + a_l b_h), one wave per query tile (a workgroup is four
 * query tiles; a wave runs the whole contraction and owns all ten output tiles).  out [B,N,feat] receives only the o_pt columns
 * (H*c_hidden ..); the o columns are written as packed planes (k-steps 16 h .. 16 h + 15 of an activation with out_xp_ksteps
 * k-steps per row: the input of linear_out); logits_out / stats_out as s2s_ipa_attention (consumed by s2s_ipa_opair).
 * ANY n_res (ipa.py:183-257 has one code path for every length): with n_pad = n_res rounded up to 32, the fragment arrays, q2 and k2
 * hold n_pad rows PER SAMPLE (row tile = sample * n_pad/32 + tile):
 *   q_xp / k_xp from s2s_node_linear and v_vf from s2s_node_linear_vfrag, both with n_rows = n_samples * n_pad and the row map
 *   (map_pad = n_pad, map_src = n_res) when n_pad != n_res; points from s2s_ipa_prep_points_f16 (padded rows: zero points,
 *   k2 = -1e9, so a padded key never carries probability -- exactly the un-padded softmax).
 * attn_bias stays [B,H,n_res,n_res]; when n_pad != n_res logits_out must be a SEPARATE [B,H,n_pad,n_pad] buffer (s2s_ipa_opair:
 * logits_ld = n_pad); stats_out [B,H,n_res,2], out [B,n_res,feat] and out_xp (row tiles of the flat [B n_res] rows) are not padded.
 *
 * FOLDED PROJECTIONS (the default host path, str2str_amd/models/net/ipa.py fold_ipa_weights; ipa.py:131-143,183-190,229-252 of the
 * reference with the weights regrouped).  With q = W_q s_i + b_q, k = W_k s_j + b_k per head, q.k = s_j . (W_k^T W_q s_i + W_k^T b_q)
 * + terms that depend on i only and cancel in the softmax over j; and sum_j a_ij v_j = W_v (sum_j a_ij s_j) + b_v as the
 * probabilities sum to one.  So with c_s = c_hidden = 256 the attention can read the block's input s as the K AND the V operand of
 * every head: q' = (W_k^T W_q) s + W_k^T b_q is the only scalar projection left (linear_k / linear_v are never evaluated; W_v and
 * b_v move into linear_out's weight and bias), and the kernel aggregates s instead of v.  n_kv_heads = 1 selects that operand
 * layout: k_xp = packed planes of s [rows/32][16][2][64][8] (s itself when n_res % 32 == 0, else k_shared below), v_vf =
 * [rows/32][8][2][2][64][8] (v_shared below); n_kv_heads = n_heads is the per-head layout above.
 * Short chains with the shared operands (n_pad <= 64: one or two key tiles per sample) run on a second kernel behind the same entry
 * point: one wave per (sample, head, query tile), no LDS and no barriers -- the streaming kernel's workgroup of four query tiles of
 * one (sample, head) repeats work on three / two of its waves there.
 * s2s_ipa_prep_points_f16 with s_xp != NULL (n_heads = 8) writes those shared operands in the same launch: v_shared always,
 * k_shared (rows gathered into the padded per-sample layout) when n_res % 32 != 0; NULL s_xp skips the step. */
int s2s_ipa_prep_points_f16(const float* rigids7, const float* q_pts_lin, const float* kv_pts_lin, const float* head_w_scaled,
                            void* qp_xp, void* kp_xp, void* vp_vf, float* q2, float* k2, int n_samples, int n_res, int n_heads,
                            int n_qk_points, int n_v_points, int c_hidden, const void* s_xp, void* k_shared, void* v_shared,
                            int* range_words, void* stream);
int s2s_ipa_attention_f16w(const void* q_xp, const void* k_xp, const void* v_vf, const void* qp_xp, const void* kp_xp,
                             const void* vp_vf, const float* q2, const float* k2, const float* attn_bias, float* logits_out,
                             float* stats_out, const float* mask, const float* rigids7, float* out, void* out_xp,
                             int out_xp_ksteps, int n_samples, int n_res, int n_heads, int c_hidden, int n_qk_points,
                             int n_v_points, int c_pair_z, float inf, float eps, int n_kv_heads, void* stream);

/* The pair term of InvariantPointAttention.forward (src/models/net/ipa.py:253-257):
 *   o_pair[b,i,h,:] = sum_j softmax_j(logits[b,h,i,:])[j] * pair_z[b,i,j,:]
 * from the logits / statistics s2s_ipa_attention stored, streaming pair_z [B,N,N,c_pair_z] once for all heads;
 * written to out[(b*N+i)*out_row_stride + out_col_offset + h*c_pair_z + c]  (H = 8, c_pair_z = 32).
 * logits_ld: rows per (sample, head) slab and row stride of ``logits`` ([B,H,ld,ld]; 0 = n_res; the padded length when
 * s2s_ipa_attention_f16w wrote them for a ragged n_res). */
int s2s_ipa_opair(const float* logits, const float* stats, const float* pair_z, float* out, int n_samples, int n_res,
                  int n_heads, int c_pair_z, int out_row_stride, int out_col_offset, int logits_ld, void* stream);

/* ---- Rigid frames ---- */

/* Rigid.compose_q_update_vec (src/common/rigid_utils.py:1042-1066, :590-619, :268-277).
 *   rigids7 [M,7], update6 [M,6], mask [M], out7 [M,7] (may alias rigids7). */
int s2s_rigid_compose_update(const float* rigids7, const float* update6, const float* mask, float* out7,
                             long long n_frames, int update_ld, void* stream);   /* update_ld: floats between consecutive update rows (>= 6): the
                                                                                    BackboneUpdate layer's padded [n, 32] output is read in place */

/* TorsionAngleHead's normalisation (src/models/net/layers.py:199-213: u / sqrt(max(u0^2 + u1^2, eps)), normalize != 0) and / or
 * DenoisingNet's blend with the input torsion under the fixed mask (denoising_ipa.py:193-195: gt * fixed + pred * (1 - fixed),
 * gt_sin_cos != NULL: row r at gt_sin_cos + r * gt_row_stride, fixed_mask [n_rows]).  u: rows of u_ld >= 2 floats (the head's padded
 * output is read in place); out2 [n_rows, 2]. */
int s2s_torsion_head(const float* u, int u_ld, int normalize, const float* gt_sin_cos, long long gt_row_stride, const float* fixed_mask,
                     float eps, float* out2, long long n_rows, void* stream);

/* TranslationIPA scale_rigids / unscale_rigids (src/models/net/ipa.py:288-292): translation * scale,
 * or translation / scale (true division) when divide != 0. */
int s2s_rigid_scale_trans(const float* rigids7, float* out7, long long n_frames, float scale, int divide, void* stream);

/* Upload the idealised-geometry tables used by s2s_frames_to_backbone to the current device (host pointers; synchronous;
 * call once per device).  Values: src/common/residue_constants.py:775-852 via all_atom.py:13-18. */
int s2s_set_backbone_tables(const float* pos_21x5x3, const float* mask_21x5, const int* is_psi_group_21x5,
                            const float* default_frames_21x2x4x4);

/* compute_backbone (src/common/all_atom.py:141-173).  rigids7 [M,7] (Angstrom), psi_sincos [M,2],
 * aatype [M] int64 or NULL; atom14_bb5 [M,5,3] (N,CA,C,O,CB) or NULL; atom37 [M,37,3] or NULL. */
int s2s_frames_to_backbone(const float* rigids7, const float* psi_sincos, const long long* aatype, float* atom14_bb5,
                           float* atom37, long long n_frames, void* stream);

/* ---- One reverse-diffusion geometry step ---- */

/* FrameDiffuser.score + FrameDiffuser.reverse + Rigid.to_tensor_7
 * (src/models/score/frame.py:109-143, :153-210; so3.py:274-309, :333-370; r3.py:79-137).
 *   x0_7 [B,N,7] predicted frames, xt_7 [B,N,7] current frames, mask/diffuse_mask [B,N],
 *   params8 [B,8] float: sigma(bin), g_rot^2, exp(-beta/2), 1-exp(-beta), b(t), g_trans^2, g_rot, g_trans
 *   z_rot,z_trans [B,N,3] double noise (only read when probability_flow == 0),
 *   rot_score_in/trans_score_in [B,N,3] double or NULL: when given, the score stage is skipped and
 *   these are used (FrameDiffuser.reverse called with caller-provided scores; x0_7 may be NULL),
 *   next7 [B,N,7] or NULL (score only); rot_score_out/trans_score_out [B,N,3] double or NULL.
 *   center_trans: 0 = off, 1 = centre of mass over all N residues (reference behaviour), 2 = over the
 *   residues with mask > 0 only (padded mixed-length batches).
 *   dt = 1 / int(num_timesteps * T) of the trajectory (diffusion_module.py:267); dt_per_sample [B] double or NULL: one step size
 *   per sample instead, for batches that hold trajectories of different t_delta (sampler.forward_backward_deltas). */
int s2s_se3_step(const float* x0_7, const float* xt_7, const float* mask, const float* diffuse_mask,
                 const float* params8, const double* z_rot, const double* z_trans,
                 const double* rot_score_in, const double* trans_score_in, float* next7,
                 double* rot_score_out, double* trans_score_out, int n_samples, int n_res, double dt,
                 const double* dt_per_sample, double coordinate_scaling, int probability_flow, int center_trans,
                 double noise_scale, void* stream);

/* The embedder's per-evaluation assembly in one launch (EmbeddingModule.forward, src/models/net/denoising_ipa.py:107-136: the first
 * Linear of the node MLP and of the edge MLP on [timestep embedding | fixed-mask column | positional block]).
 *   t_img [t_img_rows, 512] = first-layer image of the timestep embedding + bias: [node MLP 256 | edge row part 128 | edge column part 128];
 *          t_img_rows = 1: one timestep for the whole chunk, = n_rows / n_res: one row per sample (trajectories of different t in a batch)
 *   node_const [node_const_rows, 256] (rows = n_rows, or n_res when every sample shares it): fixed-mask + positional terms of the node MLP
 *   fa [n_rows,128], fb (column-blocked [B,32,n_res,4] when b_col_blocked, else [n_rows,128]): fixed-mask terms of the edge MLP
 *   -> h = relu(t_img[0:256] + node_const) as packed planes (h_xp) or fp32 [n_rows,256] (h_f32; exactly one of the two),
 *      node_a = t_img[256:384] + fa, node_b = t_img[384:512] + fb: the operands of s2s_node_linear / s2s_edge_embed(_f16x3). */
int s2s_embed_assemble(const float* t_img, long long t_img_rows, const float* node_const, long long node_const_rows, const float* fa, const float* fb,
                       long long n_rows, int n_res, void* h_xp, float* h_f32, float* node_a, float* node_b, int b_col_blocked,
                       int* range_words, void* stream);

/* ---- Per-node dense layers (split-f16 MFMA "f16x3", fp32-equivalent; see s2s_edge_transition_f16x3) ----
 * Activations travel between these layers as PACKED PLANES ("XP"): for X [M, K],
 *   XP[rt = row/32][ks = K/16][plane 2][lane 64][8] f16, lane = 32 g + (row & 31),
 *   element j = plane of X[row][32 (ks>>1) + (r&3) + 8 (r>>2) + 4 g], r = 8 (ks&1) + j;
 * planes = the f16 pair (x_h = rn16(x), x_l = rn16(x - x_h)); the attention kernel takes the same planes.  Rows past M inside the
 * last row tile are zero. */

/* fp32 row-major x [n_rows, ld], columns col0 .. col0 + n_cols (n_cols % 32 == 0), optionally scaled per row, -> k-steps
 * xp_kstep0 .. of an XP buffer holding xp_ksteps k-steps (concatenation along K = k-step ranges). */
int s2s_pack_planes(const float* x, long long n_rows, int ld, int col0, int n_cols, void* xp, int xp_ksteps, int xp_kstep0,
                    const float* row_scale, int* range_words, void* stream);

/* One nn.Linear of the node stream with its surrounding elementwise ops (reference: Linear src/models/net/layers.py:64-124;
 * call sites ipa.py:131-171 (q/kv/points), :259-266 (linear_out), :343-366 (LayerNorm, skip, transformer, linear, transitions),
 * layers.py:128-145,176,188-241; torch.nn.TransformerEncoderLayer's projections and feed-forward):
 *     v = acc * pre_scale[row] + bias;  relu;  v *= pre_mask[row];  v += residual[row, col];  LayerNorm(v) over the n_out
 *     columns (gamma/beta given; needs n_out == 32 * tiles_per_block);  v *= post_mask[row]
 *   xp: packed planes of the input [n_rows, k_in]; w_packed: ops.pack_node_weight(W [n_out, k_in], tiles_per_block);
 *   outputs: out_f32[row * out_ld + out_col0 + col] and/or the packed planes of the result as k-steps out_xp_kstep0 .. of an XP
 *   buffer with out_xp_ksteps k-steps (the input format of the next layer and of s2s_ipa_attention_f16w).
 *   Any pointer may be NULL to skip that step.
 *   Row map (map_pad > 0; only with bias / relu / LayerNorm epilogues): n_rows counts OUTPUT rows = n_samples * map_pad, and output
 *   row (sample, n) reads input row sample * map_src + min(n, map_src - 1) -- the per-sample padding to whole 32-row tiles that
 *   s2s_ipa_attention_f16w wants of its q / k / v operands for a ragged n_res (map_src = n_res, map_pad = n_res rounded up to 32). */
int s2s_node_linear(const void* xp, const void* w_packed, const float* bias, long long n_rows, int k_in, int n_out,
                    int tiles_per_block, const float* pre_scale, int relu, const float* pre_mask, const float* residual,
                    int residual_ld, const float* ln_gamma, const float* ln_beta, float ln_eps, const float* post_mask,
                    float* out_f32, int out_ld, int out_col0, void* out_xp, int out_xp_ksteps, int out_xp_kstep0,
                    int map_pad, int map_src, int* range_words, void* stream);

/* The same layer, same epilogue, on EXACT fp32 MFMA: x fp32 row-major [n_rows, x_ld] (its first k_in columns, k_in % 8 == 0),
 * w_packed = ops.pack_node_weight_f32(W, tiles_per_block): [n_out/(32 TG)][k_in/8][TG][64][4] fp32 in the pack_weight lane order,
 * out_f32 required.  No planes, no range limit: the node stream of the "f32" arithmetic. */
int s2s_node_linear_f32(const float* x, int x_ld, const float* w_packed, const float* bias, long long n_rows, int k_in, int n_out,
                        int tiles_per_block, const float* pre_scale, int relu, const float* pre_mask, const float* residual,
                        int residual_ld, const float* ln_gamma, const float* ln_beta, float ln_eps, const float* post_mask,
                        float* out_f32, int out_ld, int out_col0, void* stream);

/* The same GEMM with the operands swapped, for a projection whose output is consumed as the A operand of a later product over
 * its ROWS (the value projection of InvariantPointAttention, ipa.py:132-141, consumed by the PV step): the result (+ bias) is
 * stored as MFMA A fragments of f16 pairs  out_vf[row tile (32 rows)][head][column tile (32 cols) in head][k-step u (16 rows)]
 * [plane 2][lane 64][8], element j of lane (column c, half h) = row (r&3) + 8 (r>>2) + 4 h, r = 8 u + j, of the tile.  w_packed as
 * for s2s_node_linear with tiles_per_block = 8.  map_pad / map_src: the row map of s2s_node_linear. */
int s2s_node_linear_vfrag(const void* xp, const void* w_packed, const float* bias, long long n_rows, int k_in, int n_out,
                          int tiles_per_head, void* out_vf, int map_pad, int map_src, int* range_words, void* stream);

/* Up to six INDEPENDENT node layers (bias / ReLU epilogues, no residual / LayerNorm / masks) in one launch -- the five projections of an
 * IPA block (linear_q, the k and v halves of linear_kv, linear_q_points, linear_kv_points: ipa.py:131-171) read the same activations
 * and nothing of each other.  Each problem is the argument list of s2s_node_linear (bias / pre_scale / relu epilogue; tiles_per_block 1, 2,
 * 4, 5, 6, 8 or 10) or, with vfrag_tiles_per_head > 0, of s2s_node_linear_vfrag.  Besides the IPA projections the trunk runs this way
 * the four skip_embed layers (they all read the embedder's output) and, per block, BackboneUpdate + the EdgeTransition's per-node
 * parts (+ the torsion head's first layer after the last block): layers of one input, one launch. */
typedef struct s2s_node_problem {
    const void* xp; const void* w_packed; const float* bias;
    long long n_rows; int k_in, n_out, tiles_per_block;
    int vfrag_tiles_per_head;
    float* out_f32; int out_ld, out_col0;
    void* out_xp; int out_xp_ksteps, out_xp_kstep0;
    void* out_vf;
    int map_pad, map_src, relu;
    const float* pre_scale;   /* [n_rows] or NULL: row scale applied to the accumulator before the bias (s2s_node_linear) */
} s2s_node_problem;
int s2s_node_linear_multi(const s2s_node_problem* problems, int n_problems, int* range_words, void* stream);

/* A chain of 2 .. 4 layers of one output width (256 or 320) in one launch: every layer but the last is relu?(W x + b), the last one
 * has the epilogue and outputs of s2s_node_linear.  The hidden activations stay in registers (the accumulator layout of a layer is the
 * operand layout of the next); bit for bit the separate launches.  w_packed: ops.pack_node_weight(W, width / 32).
 * The FIRST layer may contract over k_in0 != width columns (320 -> 256) and may add a residual (mid_residual [n_rows, ld]) and store its
 * fp32 result (mid_out_f32 [n_rows, ld]) -- which may then be the last layer's ``residual``: trunk.linear + NodeTransition
 * (src/models/net/ipa.py:358-359, layers.py:128-145) as one launch.  The first layer may also carry a LayerNorm of its own behind that
 * residual (mid_ln_gamma / mid_ln_beta [width], mid_ln_eps; NULL = none): an nn.TransformerEncoderLayer's post-attention half --
 * out_proj + residual + norm1, linear1, relu, linear2 + residual (= the stored norm1 output) + norm2 (ipa.py:312-317) -- as one launch.
 * Also: the embedder's node MLP (denoising_ipa.py:113-120). */
typedef struct s2s_chain_layer { const void* w_packed; const float* bias; int relu; } s2s_chain_layer;
int s2s_node_chain(const void* xp, const s2s_chain_layer* layers, int n_layers, long long n_rows, int width, int k_in0,
                   const float* mid_residual, int mid_residual_ld, float* mid_out_f32, int mid_out_ld, const float* mid_ln_gamma,
                   const float* mid_ln_beta, float mid_ln_eps, const float* pre_mask, const float* residual, int residual_ld, const float* ln_gamma, const float* ln_beta, float ln_eps,
                   const float* post_mask, float* out_f32, int out_ld, int out_col0, void* out_xp, int out_xp_ksteps,
                   int out_xp_kstep0, int* range_words, void* stream);

/* The LayerNorm (+ post mask) half of a node layer on its own: fp32 rows x [n_rows, x_ld] (n_cols = 256 or 320) -> out_f32 and / or packed
 * planes, with the epilogue code of s2s_node_linear -- a layer run as s2s_node_linear(ln = NULL, out_f32 = x) followed by this call
 * equals the fused layer bit for bit.  For long contractions on few rows (linear_out, K = 2688, ipa.py:259-266): the GEMM can then run
 * in narrow column blocks instead of one block per row tile. */
int s2s_row_layernorm(const float* x, int x_ld, long long n_rows, int n_cols, const float* ln_gamma, const float* ln_beta, float ln_eps,
                      const float* post_mask, float* out_f32, int out_ld, int out_col0, void* out_xp, int out_xp_ksteps,
                      int out_xp_kstep0, int* range_words, void* stream);

/* Self-attention core of the trunk's TransformerEncoderLayer (src/models/net/ipa.py:312-317,357; torch.nn.MultiheadAttention with
 * d_model = n_heads * head_dim, head_dim = 80): softmax(q k^T / sqrt(head_dim) + key_bias[j]) v per (sample, head), exact fp32 MFMA.
 *   qkv [B*N, 3*D] fp32 = in_proj output (q | k | v); key_bias [B,N] or NULL: added to the logits of key j (PyTorch's float
 *   key-padding-mask semantics; -inf removes a key); out_f32 [B*N, D] and/or out_xp = packed planes of it (see above). */
int s2s_encoder_attention(const float* qkv, const float* key_bias, float* out_f32, void* out_xp, int n_samples, int n_res,
                          int n_heads, int head_dim, int* range_words, void* stream);

/* The same operator on split-f16 MFMA ("f16x3", the default arithmetic): q, k, v and the probabilities as f16 pairs, three products
 * per block, fp32 softmax and accumulation; q, k, v feed the range guard.  Same arguments. */
int s2s_encoder_attention_f16x3(const float* qkv, const float* key_bias, float* out_f32, void* out_xp, int n_samples, int n_res,
                          int n_heads, int head_dim, int* range_words, void* stream);

/* ---- Forward process / prior, once per trajectory ---- */

/* FrameDiffuser.forward_marginal (src/models/score/frame.py:36-107; so3.py:244-272, :315-331, :13-19; r3.py:49-74) or, with
 * rigids0_4x4 == NULL, FrameDiffuser.sample_prior (frame.py:212-255), followed by Rigid.to_tensor_7.
 *   rigids0_4x4 [B,N,4,4] starting frames (Angstrom) or NULL; noise drawn by the caller: z_axis [B,N,3] ~ N(0,1) (rotation
 *   axis), u01 [B,N] ~ U[0,1) (inverse CDF of the IGSO(3) angle), z_trans [B,N,3] ~ N(0,1);
 *   cdf_rows [R,n_omega] double (so3.py:185-187) and cdf_row_of_sample [B] (row per sample = sigma bin of its t),
 *   omega_grid [n_omega] (SO3Diffuser.discrete_omega); params2 [B,2] = exp(-marginal_b_t/2), sqrt(1-exp(-marginal_b_t));
 *   diffuse_mask [B,N] or NULL (= all ones); out rigids_t7 [B,N,7]. */
int s2s_forward_marginal(const float* rigids0_4x4, const float* z_axis, const float* u01, const float* z_trans,
                         const double* cdf_rows, const int* cdf_row_of_sample, const float* omega_grid, int n_omega,
                         const float* params2, const float* diffuse_mask, float coordinate_scaling, float* rigids_t7,
                         int n_samples, int n_res, void* stream);

/* ---- Ensemble metrics on the device (src/metrics/metrics.py) over CA coordinates [n, L, 3] float32 ---- */

/* Per sample: CA pairs (|i-j| > k_exclusion) closer than clash_bar (metrics.py:80-105), the largest adjacent CA-CA distance
 * (:12-23; bonding_validity :124-137 compares it with the reference ensemble's), the radius of gyration (:53-77, float64). */
int s2s_ca_sample_stats(const float* ca, int n_samples, int n_res, float clash_bar, int k_exclusion, int* n_clash,
                        float* adjacent_max, double* radius_of_gyration, void* stream);

/* pairwise_distance_ca (metrics.py:38-50): out [n_samples, D] float32, D = (L-offset)(L-offset+1)/2 upper-triangular CA distances per sample
 * in np.triu_indices(L, k=offset) order, in numpy's float32 arithmetic (bit for bit): the features of js_tica (:166-200).  n_samples <= 65535. */
int s2s_ca_pairwise_distances(const float* ca, int n_samples, int n_res, int offset, float* out, void* stream);

/* js_pwd (metrics.py:140-166): per pair channel (i, j >= i + offset; np.triu_indices order) the Jensen-Shannon distance between
 * the n_bins-bin histograms (range = the reference ensemble's [min, max], numpy's float32 bin arithmetic, + pseudo_count) of the
 * predicted and the reference ensemble -> js_per_channel [(L-offset)(L-offset+1)/2] float64 (the metric is their mean).
 * ref_weights [n_ref] / pred_weights [n_pred]: per-sample float64 histogram weights (the reference's `weights=`, metrics.py:139-150;
 * NULL = all ones, both NULL = integer counts). */
int s2s_ca_pwd_js(const float* ref_ca, int n_ref, const float* pred_ca, int n_pred, int n_res, int offset, int n_bins,
                  double pseudo_count, double* js_per_channel, const double* ref_weights, const double* pred_weights, void* stream);

/* ---- Minimum RMSD under optimal rigid superposition (csrc/ensemble_rmsd.hip; no counterpart in the reference) ----
 * Convention: MSD = min over PROPER rotations R (det R = +1: a mirror image is not superposable) and translations t of
 * sum_i w_i |R a_i + t - b_i|^2 / sum_i w_i;  rmsd = sqrt(max(MSD, 0)).  weights [n_res] float32 >= 0 with a positive sum, NULL = all ones.
 * Arithmetic: the float32 coordinates are widened to float64; weighted centroids, G = sum w |x - x-bar|^2, the cross-covariance
 * H = sum w (a - a-bar)(b - b-bar)^T and the largest eigenvalue lambda of Horn's 4 x 4 quaternion matrix of H (cyclic Jacobi) are all
 * float64; MSD = (G_a + G_b - 2 lambda) / W.  n_res = 1 gives exactly 0. */

/* All pairs of two ensembles a [n_a, n_res, 3], b [n_b, n_res, 3] -> rmsd [n_a, n_b] float64 (H of 16 x 16 pairs per wave on the
 * float64 matrix instruction).  b == a with n_b == n_a is the self case: the upper triangle is computed and mirrored.  a may also be a
 * contiguous run of b's structures (a row chunk of the self matrix): the rows are then bit for bit those of the self matrix, which is
 * exactly symmetric.  workspace: caller-owned scratch of workspace_doubles >= 2 + r(n_b) + r(n_a) doubles (r(n_a) not needed in the
 * self case), r(n) = 16 ceil(n / 16) (3 * 4 ceil(n_res / 4) + 1); nothing survives the call.  n_a * n_b < 2^31 and n_a <= 16 * 65535 per
 * call (the binding chunks rows). */
int s2s_ca_rmsd_matrix(const float* a, int n_a, const float* b, int n_b, int n_res, const float* weights, double* rmsd,
                       double* workspace, long long workspace_doubles, void* stream);

/* mobile [n_mobile, n_res, 3] onto target [n_res, 3] -> rmsd [n_mobile] float64 and xform [n_mobile, 12] float64: the row-major rotation R
 * (from the normalised eigen-quaternion of lambda; any optimal rotation where the eigenspace is degenerate) followed by the translation
 * t = b-bar - R a-bar, so that R x + t maps mobile onto target. */
int s2s_ca_superpose(const float* mobile, int n_mobile, const float* target, int n_res, const float* weights, double* rmsd,
                     double* xform, void* stream);

/* out[s, m] = float32(R_s points[s, m] + t_s) for points [n_samples, n_points, 3] float32 (CA: n_points = n_res; atom37: 37 n_res) and
 * xform [n_samples, 12] as above, accumulated in float64; out may alias points. */
int s2s_apply_xform(const float* points, const double* xform, int n_samples, long long n_points, float* out, void* stream);

/* ---- TM-score under the identity correspondence (csrc/ensemble_tm.hip; no counterpart in the reference) ----
 * TM(a, b) = max over the evaluated superpositions (R proper, t) of (1/L) sum_i 1 / (1 + |R a_i + t - b_i|^2 / d0^2), L = n_res, residue i
 * of a against residue i of b (the TMscore program's convention, not TM-align's), float64 arithmetic on the widened float32 coordinates.
 * d0 <= 0 selects d0(L) = max(0.5, 1.24 cbrt(L - 15) - 1.8) for L > 15, else 0.5.
 * Search (fixed; no data-dependent termination): for every seed window (s, n) start from weights 1 on residues s .. s+n-1 and 0 elsewhere,
 * then 33 times: weighted Kabsch of a onto b (proper rotation from the eigen-quaternion of Horn's 4 x 4, cyclic Jacobi), evaluate the score,
 * w_i <- f_i^2.  A reweighting never lowers the score; the result is the maximum over all seeds and evaluations, a lower bound of the true
 * optimum and a continuous function of the coordinates.  Seeds: (0, L); then for div in (2, 4): n = max(L / div, 4), skipped if n >= L,
 * starts 0, n/2, 2 (n/2), ... while s + n <= L, plus (L - n, n) if the last window stops short of L (at most 16).  n_res = 1 gives exactly 1. */
#define S2S_TM_MAX_RES 800   /* the coordinates of a 4 x 4 tile of pairs stay in LDS: 192 B per residue */

/* All pairs of a [n_a, n_res, 3] and b [n_b, n_res, 3] -> tm [n_a, n_b] float64.  b == a with n_b == n_a is the self case: pairs i <= j are
 * evaluated and mirrored (exactly symmetric; the diagonal comes from its own pair).  a may also be a contiguous run of b's structures (a row
 * chunk of the self matrix): the rows are then bit for bit those of the self matrix.  No scratch.  Per call n_a * n_b < 2^31,
 * n_b <= 4 * 65535 and n_res <= S2S_TM_MAX_RES (the binding chunks rows). */
int s2s_ca_tm_matrix(const float* a, int n_a, const float* b, int n_b, int n_res, double d0, double* tm, void* stream);

/* mobile [n_mobile, n_res, 3] onto target [n_res, 3] -> tm [n_mobile] (the s2s_ca_tm_matrix entry of the pair) and xform12 [n_mobile, 12]
 * in the layout of s2s_ca_superpose (s2s_apply_xform consumes it): the superposition that scored the maximum (the first seed to reach it). */
int s2s_ca_tm_superpose(const float* mobile, int n_mobile, const float* target, int n_res, double d0, double* tm, double* xform12,
                        void* stream);

/* ---- lDDT: the superposition-free local distance difference test on CA atoms (csrc/ensemble_lddt.hip; the reference's own definition,
 * src/models/loss.py:384-460, is its training-time `lddt` / `lddt_ca`; Mariani et al. 2013) ----
 * For a reference structure a and a model b (n_res residues, residue i matched to residue i), d_x(i, j) = |x_i - x_j|:
 *   P(a)      = {(i, j) ordered : |i - j| >= min_seq_sep, d_a(i, j) < cutoff}          (the environment comes from the FIRST argument)
 *   hits      = sum over (i, j) in P(a) of #{t in {0.5, 1, 2, 4} : |d_a(i, j) - d_b(i, j)| < t}
 *   lDDT(a->b) = hits / (4 |P(a)|),  1.0 when P(a) is empty (the limit of the reference's eps / eps; it covers n_res = 1).
 * Per residue the sums run over the pairs of a fixed i; a residue without an included partner scores 1.0.  Not symmetric.
 * Arithmetic: the float32 coordinates are widened to float64 and every distance is float64.  d_a is a square root; d_b is never formed:
 * |d_a - d_b| < t is evaluated as d_b^2 < (d_a + t)^2 and (d_a - t < 0 or d_b^2 > (d_a - t)^2).  hits and |P| are integers and the score is one
 * float64 division of them, so a value does not depend on the launch it is computed in.  A comparison with NaN is false: such a pair is
 * neither included nor hit.  The reference's defaults are cutoff = 15.0 A and min_seq_sep = 1 (i != j).
 * workspace (both entry points): caller-owned scratch, 8-byte aligned, of at least S2S_LDDT_WORKSPACE_BYTES(n_a, n_res) bytes (n_a = 1 for the
 * per-residue form): per reference structure the list of its included pairs i > j -- c = 2 ceil(n_res (n_res - 1) / 4) slots of a float64
 * d_a and an int32 (i << 16 | j) -- its length, and the partner count of every residue.  Nothing survives the call. */
#define S2S_LDDT_MAX_RES 1024   /* a tile of 8 models stays in LDS as float32: 96 B per residue */
#define S2S_LDDT_LIST_SLOTS(n_res) (((long long)(n_res) * ((long long)(n_res) - 1) / 2 + 1) / 2 * 2)
#define S2S_LDDT_WORKSPACE_BYTES(n_a, n_res) ((long long)(n_a) * (12 * S2S_LDDT_LIST_SLOTS(n_res) + 8 + 4 * (long long)(n_res)))

/* Every structure of a [n_a, n_res, 3] as the reference of every structure of b [n_b, n_res, 3] -> lddt [n_a, n_b] float64 in [0, 1].
 * cutoff positive and finite, min_seq_sep >= 1, n_res <= S2S_LDDT_MAX_RES, n_a * n_b < 2^31 per call (the binding chunks rows).  b == a is
 * allowed and not special-cased: the diagonal is exactly 1.0 because every pair of a structure hits under all four thresholds. */
int s2s_ca_lddt_matrix(const float* a, int n_a, const float* b, int n_b, int n_res, double cutoff, int min_seq_sep, double* lddt,
                       void* workspace, long long workspace_bytes, void* stream);

/* model [n_model, n_res, 3] against the reference target [n_res, 3] -> per_res [n_model, n_res] and total [n_model] float64; total is bit for
 * bit the s2s_ca_lddt_matrix entry of (target, model). */
int s2s_ca_lddt_per_residue(const float* model, int n_model, const float* target, int n_res, double cutoff, int min_seq_sep,
                            double* per_res, double* total, void* workspace, long long workspace_bytes, void* stream);

/* ---- Backbone violations: is the sampled backbone chemically possible?  (csrc/ensemble_violations.hip; the definition is the reference's
 * find_structural_violations / compute_violation_metrics, src/models/loss.py:714-1017, 1237-1314 -- the AlphaFold structural-violation terms --
 * restricted to the five atoms the sampler writes) ----
 * Per structure of atoms [n, n_res, 5, 3] (atom14 slots N, CA, C, O, CB), with atom_exists [n_res, 5] (bytes, != 0: the atom exists; GLY has
 * no CB), aatype [n_res] (the reference's residue order: PRO = 14) and residue_index [n_res] shared by the n structures:
 *  1. Connections k -> k + 1 (between_residue_bond_loss), eps = 1e-6 inside every square root, t = tolerance_factor:
 *       c_n = sqrt(eps + |C_k - N_k+1|^2),  e_cn = sqrt(eps + (c_n - g)^2), g / sigma = 1.329 / 0.014, or 1.341 / 0.016 when k + 1 is PRO;
 *       e_cacn = sqrt(eps + (cos(CA_k - C_k, N_k+1 - C_k) + 0.4473)^2), e_cnca = sqrt(eps + (cos(C_k - N_k+1, CA_k+1 - N_k+1) + 0.5203)^2),
 *       the vectors divided by their sqrt(eps + |.|^2) lengths;  loss = max(e - t w, 0) and violated = e > t w with w = sigma, 0.014, 0.0353.
 *     The width of the CA-C-N term is the C-N bond length's 0.014, not the 0.0311 of the cosine: the reference's own choice (loss.py:809), kept.
 *     A term counts where residue_index[k + 1] - residue_index[k] == 1 and its atoms exist (C_k, N_k+1; + CA_k; + CA_k+1).
 *     losses[., 0 .. 2] = sum of the counted losses / (number counted + 1e-6); per_residue_loss[., r] = half the UNMASKED loss sum
 *     (the three losses, whether counted or not) of the connections r - 1 -> r and r -> r + 1; bond_mask[., r] = 1 if either connection is violated.
 *  2. Clashes (between_residue_clash_loss): the pairs of existing atoms of residues with residue_index[i] < residue_index[j], except C_i - N_j
 *     where residue_index[j] == residue_index[i] + 1.  d = sqrt(1e-10 + |.|^2), bound = r_a + r_b - clash_tolerance with r = 1.7 (C),
 *     1.55 (N), 1.52 (O).  A pair clashes iff d < bound, its loss is max(bound - d, 0).  losses[., 3] = sum / (1e-6 + number of pairs);
 *     clash_atom_mask[., r, a] = 1 if the atom is in a clashing pair; n_clash_pairs = the number of clashing pairs.
 *  3. fractions[., 0 .. 3] (compute_violation_metrics; masked_mean's eps 1e-4): residues with bond_mask / (1e-4 + n_res); residues with a
 *     clashing atom / (1e-4 + n_res); residues with either / (1e-4 + n_res); connections without a gap whose CA atoms exist and whose
 *     sqrt(1e-6 + |CA_k - CA_k+1|^2) - 3.80209737096 > 1.5, over (1e-4 + the number of such connections).
 * Left out: the reference's within-residue term (its bounds table is not in its tree, and inside a residue the backbone is an ideal rigid
 * group by construction), the disulfide exemption (no SG), side-chain slots, gradients.  The reference's defaults: tolerance_factor = 12,
 * clash_tolerance = 1.5.
 * Arithmetic: the float32 coordinates are widened and everything is float64, one rounding per operation (no contraction).  A residue pair is
 * expanded into its atom pairs only if d(CA_i, CA_j) < rho_i + rho_j + (3.4 - clash_tolerance), rho = the largest distance of a residue's
 * existing atoms from its CA: a pair that fails cannot hold a clash, for any coordinates, so no output depends on this.  Every float64 sum
 * is formed in an order that depends on n_res alone, so a structure's outputs do not depend on the launch it is computed in.  A comparison
 * with NaN is false. */
#define S2S_VIOL_MAX_RES 1024   /* the structure's atoms stay in LDS as float64: 144 B per residue with the per-residue state */

/* No scratch.  n >= 1, 1 <= n_res <= S2S_VIOL_MAX_RES, both tolerances finite; otherwise hipErrorInvalidValue before any launch.
 * losses [n, 4] and fractions [n, 4] float64 in the order above, per_residue_loss [n, n_res] float64, bond_mask [n, n_res] and
 * clash_atom_mask [n, n_res, 5] bytes, n_clash_pairs [n] int. */
int s2s_backbone_violations(const float* atoms, int n, int n_res, const unsigned char* atom_exists, const int* aatype,
                            const int* residue_index, double tolerance_factor, double clash_tolerance, double* losses, double* fractions,
                            double* per_residue_loss, unsigned char* bond_mask, unsigned char* clash_atom_mask, int* n_clash_pairs,
                            void* stream);

/* ---- Secondary structure and backbone torsions: what is each conformation?  (csrc/ensemble_ss.hip; Kabsch & Sander, Biopolymers 22
 * (1983) 2577; no counterpart in the reference beyond its torsion angles) ----
 * Per structure of atoms [n, n_res, 5, 3] (atom14 slots N, CA, C, O, CB; CB is not used), with aatype [n_res] (the reference's residue
 * order: PRO = 14) and residue_index [n_res] shared by the n structures.  Indices i, j are positions 0 .. L - 1 in the chain, L = n_res.
 *  Connection and segments.  Residue j is connected iff residue_index[j] == residue_index[j - 1] + 1 (residue 0 never is).  Segments are
 *     the maximal runs of connected residues; a range a .. b is unbroken iff residues a + 1 .. b are connected.
 *  Amide hydrogen.  Residue j has one iff it is connected and not PRO:  H_j = N_j + (C_j-1 - O_j-1) / |C_j-1 - O_j-1|.
 *  Energy of C=O of i accepting N-H of j:  E(i -> j) = 27.888 (((1 / r(O_i, N_j) + 1 / r(C_i, H_j)) - 1 / r(O_i, H_j)) - 1 / r(C_i, N_j))
 *     kcal/mol; if any of the four distances is below 0.5 A, E = -9.9 (DSSP's rule).
 *  H-bond.  hb(i -> j) iff j has H, j != i, j != i + 1, |CA_i - CA_j| < 9.0 and E(i -> j) < -0.5.  The 9.0 A test is DSSP's own prefilter
 *     and part of the definition.  DEPARTURE 1 from the DSSP program: the threshold alone decides; there is no bookkeeping of the two
 *     best bonds per group.
 *  n-turn, n = 3, 4, 5.  turn_n(i) iff i + n < L, i .. i + n is unbroken and hb(i -> i + n).
 *  Bridge, for 1 <= i, j <= L - 2, |i - j| >= 3, i - 1 .. i + 1 and j - 1 .. j + 1 unbroken:
 *     par(i, j)  = [hb(i - 1 -> j) and hb(j -> i + 1)] or [hb(j - 1 -> i) and hb(i -> j + 1)];
 *     anti(i, j) = [hb(i -> j) and hb(j -> i)] or [hb(i - 1 -> j + 1) and hb(j - 1 -> i + 1)].
 *  Ladder.  i is in a ladder iff for some j: par(i, j) and (par(i + 1, j + 1) or par(i - 1, j - 1)), or
 *     anti(i, j) and (anti(i + 1, j - 1) or anti(i - 1, j + 1)).  DEPARTURE 2: the beta-bulge rule, which merges two ladders across a
 *     short gap, is left out.
 *  Bend at i, for 2 <= i <= L - 3 with i - 2 .. i + 2 unbroken, iff cos(CA_i - CA_i-2, CA_i+2 - CA_i) < cos 70 degrees.
 *  States.  From '-', in this order:  1. 'B' for a residue in any bridge, then 'E' over it for a residue in a ladder;  2. 'H' on i .. i + 3
 *     wherever turn_4(i - 1) and turn_4(i), unconditionally;  3. 'G' on i .. i + 2 wherever turn_3(i - 1) and turn_3(i) and all three
 *     residues are '-' or 'G';  4. 'I' on i .. i + 4 wherever turn_5(i - 1) and turn_5(i) and all five are '-' or 'I';  5. 'T' on
 *     i + 1 .. i + n - 1 of every n-turn where the residue is still '-';  6. 'S' at a bend where the residue is still '-'.  Steps 3 and 4
 *     only add the letter they tolerate, so each is decided against the state after the step before it.
 *  N-H -> O column.  hb_energy[j] = the lowest E(i -> j) over the acceptors i that pass everything but the energy test (j has H, j != i,
 *     j != i + 1, |CA_i - CA_j| < 9.0), hb_partner[j] that i, the lowest among equals; 0.0 and -1 when there is none.
 *  Torsions in radians in (-pi, pi], IUPAC sign, dihedral(p0, p1, p2, p3) = atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3)) with
 *     b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2:  phi_i = (C_i-1, N_i, CA_i, C_i), psi_i = (N_i, CA_i, C_i, N_i+1),
 *     omega_i = (CA_i-1, C_i-1, N_i, CA_i), stored at residue i (the reference's "pre-omega").  phi_i and omega_i are defined iff i is
 *     connected, psi_i iff i + 1 is; an undefined angle is 0.0.
 * Arithmetic: the float32 coordinates are widened and everything is float64, one rounding per operation (no contraction); a distance is
 * sqrt((dx dx + dy dy) + dz dz).  A comparison with NaN is false.  A structure's outputs depend on its own coordinates alone. */
#define S2S_SS_MAX_RES 704   /* four atoms and H as float64 planes plus the bond relation, L x ceil(L / 64) words: 150 KiB of LDS */

/* No scratch.  n >= 1, 1 <= n_res <= S2S_SS_MAX_RES; otherwise hipErrorInvalidValue before any launch.  ss [n, n_res] bytes (the ASCII
 * letters - B E H G I T S), n_hbonds [n] int (the pairs with hb(i -> j)), hb_energy [n, n_res] float64, hb_partner [n, n_res] int,
 * torsions [n, n_res, 3] float64 (phi, psi, omega). */
int s2s_secondary_structure(const float* atoms, int n, int n_res, const int* aatype, const int* residue_index, unsigned char* ss,
                            int* n_hbonds, double* hb_energy, int* hb_partner, double* torsions, void* stream);

/* ---- Threshold clustering of an ensemble (csrc/ensemble_cluster.hip; no counterpart in the reference) ----
 * The GROMOS algorithm (Daura et al. 1999, `gmx cluster -method gromos`) on a symmetric neighbour relation i ~ j (i ~ i always): until no
 * structure is live, the live structure with the most live neighbours (the lowest index among equals) becomes the centre of the next
 * cluster, its live neighbours (itself included) form the cluster and stop being live.  Cluster ids are in order of extraction, sizes are
 * non-increasing.
 * Bit layout: adj [n, W] 64-bit words, W = ceil(n / 64); bit (j % 64) of word (j / 64) of row i, little-endian, is i ~ j. */
#define S2S_CLUSTER_MAX_N 65536   /* structures: 512 MB of neighbour bits, and one live word per thread of the single picking workgroup */

/* values [n_rows, n] float64: rows row0 .. row0 + n_rows - 1 of an n x n matrix -> those rows of adj and their popcounts deg [n] (the
 * other rows of both are left alone).  i ~ j iff values <= cutoff (at_least == 0: distances) or values >= cutoff (at_least != 0:
 * similarities); the diagonal bit is always set, bits of columns >= n are always clear, NaN is never a neighbour. */
int s2s_cluster_adjacency(const double* values, int n_rows, int row0, int n, double cutoff, int at_least, unsigned long long* adj,
                          int* deg, void* stream);

/* Enqueues n_rounds rounds (pick + update, two launches each) of the greedy loop on the stream; init != 0 first marks all n structures
 * live.  deg [n] (the row popcounts) is consumed: it holds the LIVE neighbour counts as the loop goes.  labels [n], centres [n], sizes [n]
 * are filled as clusters are extracted; state [3] int: {live structures, clusters so far, size of the last round's cluster (0: the round
 * had nothing to do)}.  live_ws, members_ws: W words each, caller-owned, kept between calls.  A round with nothing live is a
 * no-op, so the result does not depend on n_rounds per call: the caller repeats (init = 0) until state[0] reads 0.  Once the largest live
 * count is 1 all live structures become singleton clusters, in index order, in that one round. */
int s2s_cluster_gromos(const unsigned long long* adj, int* deg, int n, int init, int n_rounds, int* labels, int* centres, int* sizes,
                       int* state, unsigned long long* live_ws, unsigned long long* members_ws, void* stream);

/* ---- Contacts on CA atoms: the contact map of an ensemble, contact order, and the fraction of native contacts Q
 * (csrc/ensemble_contacts.hip; no counterpart in the reference) ----
 * Coordinates are CA atoms [., n_res, 3] float32, residue i of one structure matched to residue i of another (the identity correspondence).
 * All arithmetic is float64, one rounding per operation (no contraction).  For residues i < j of one structure
 *   v(i, j) = (dx dx + dy dy) + dz dz,  the differences formed in float64 from the widened coordinates.
 *  Contact.  (i, j) with j - i >= min_seq_sep is a contact iff v < cutoff^2: squared form, no square root decides a contact.  A comparison
 *     with NaN is false.  The usual choice is cutoff = 8.0 A, min_seq_sep = 3.
 *  Contact map of n structures.  counts[i, j] = counts[j, i] = the number of structures in which (i, j) is a contact, int32;
 *     weighted[i, j] = weighted[j, i] = sum over the structures r, in ASCENDING r, of weights[r] [contact_r(i, j)], float64.  Both are 0
 *     inside the band |i - j| < min_seq_sep.  The probability P = counts / n, or weighted / sum of the weights, is the caller's one division.
 *  Per-structure statistics.  n_contacts[r] int32; sep_sum[r] = the sum of (j - i) over its contacts, int64.  The relative contact order
 *     (Plaxco, Simons and Baker 1998) is sep_sum / (n_res n_contacts), 0.0 for a structure without contacts: the caller forms it from the
 *     two integers.
 *  Native contact list of one structure.  All (i, j), j - i >= min_seq_sep, with v0 < native_cutoff^2, and d0 = sqrt(v0), in ascending
 *     (i, j) order.  Best, Hummer and Eaton (2013) take |i - j| > 3, i.e. min_seq_sep = 4.
 *  Q of a structure against a list of n entries.
 *     hard:  hits = #{entries : v < (lam d0)^2},  Q = hits / n                  (integer hits, one division; (lam d0)^2 is formed once per entry)
 *     soft:  Q = (1 / n) sum over the entries of 1 / (1 + exp(beta (sqrt(v) - lam d0)))        (Best, Hummer and Eaton 2013)
 *     Their values are beta = 5 / A and lam = 1.2, the lam they give for coarse-grained CA models (1.8 is their all-atom value).  Under the
 *     soft form the native scores slightly BELOW 1 against itself: every term is 1 / (1 + exp(-beta (lam - 1) d0)) < 1.  n = 0 gives 1.0 in
 *     both forms (the convention of the lDDT section for an empty set; it covers n_res <= min_seq_sep).  A structure with a NaN coordinate
 *     in an entry misses the hit and has a NaN soft Q.
 *     The soft sum is formed in an order that depends on n and on the kernel's fixed block shape alone: thread t of 256 adds the entries
 *     t, t + 256, ... in ascending order, the 64 lanes of a wave meet in an xor tree, the four waves are added in turn.  A structure's Q is
 *     therefore bit for bit the same in any launch.
 * Limits: n_res <= S2S_CONTACT_MAX_RES; CA atoms only (no CB or all-atom contacts), one sequence, no per-residue Q. */
#define S2S_CONTACT_MAX_RES 1024          /* a tile of 8 structures of the Q kernel stays in LDS as float32: 96 B per residue */
#define S2S_CONTACT_MAX_STRUCTURES 65535  /* structures per s2s_ca_contact_map call (the binding walks longer ensembles in such runs) */
#define S2S_CONTACT_LIST_SLOTS(n_res) ((long long)(n_res) > 1 ? (long long)(n_res) * ((long long)(n_res) - 1) / 2 : 1)

/* ca [n, n_res, 3] -> ADDS into counts [n_res, n_res] int32 and, with weights [n] float64 (NULL: none; then weighted must be NULL too),
 * into weighted [n_res, n_res] float64; the caller zeroes both before the first call of a map.  The upper triangle is accumulated and then
 * copied over the lower one.  Without weights the structures are split over workgroups that meet in int32 atomics.  With weights every
 * pair's sum is continued by one thread from the value the buffer holds, in ascending structure order: calls over consecutive runs of
 * structures of an ensemble give bit for bit the sum of one call.  1 <= n <= S2S_CONTACT_MAX_STRUCTURES, 1 <= n_res <=
 * S2S_CONTACT_MAX_RES, cutoff positive and finite, min_seq_sep >= 1; otherwise hipErrorInvalidValue before any launch. */
int s2s_ca_contact_map(const float* ca, int n, int n_res, double cutoff, int min_seq_sep, const double* weights, int* counts,
                       double* weighted, void* stream);

/* ca [n, n_res, 3] -> n_contacts [n] int32, sep_sum [n] int64.  No scratch.  The checks of s2s_ca_contact_map, without its limit on n. */
int s2s_ca_contact_stats(const float* ca, int n, int n_res, double cutoff, int min_seq_sep, int* n_contacts, long long* sep_sum,
                         void* stream);

/* native [n_res, 3] -> pairs [slots, 2] int32 (i, j) and d0 [slots] float64, slots >= S2S_CONTACT_LIST_SLOTS(n_res), caller-owned; the
 * first *n_pairs entries are the list, *n_pairs (device memory) is written by the kernel.  The same checks. */
int s2s_ca_native_contacts(const float* native, int n_res, double cutoff, int min_seq_sep, int* pairs, double* d0, int* n_pairs,
                           void* stream);

/* ca [n, n_res, 3] against the first n_pairs entries of (pairs, d0) -> q_soft [n], q_hard [n] float64 and hits [n] int32.  beta and lam
 * positive and finite, 0 <= n_pairs <= S2S_CONTACT_LIST_SLOTS(n_res); an entry with an index outside 0 .. n_res - 1 is skipped. */
int s2s_ca_native_q(const float* ca, int n, int n_res, const int* pairs, const double* d0, int n_pairs, double beta, double lam,
                    double* q_soft, double* q_hard, int* hits, void* stream);

/* ---- Solvent accessibility: how much of each residue, and of the chain, is exposed?  (csrc/ensemble_sasa.hip; the point test of Shrake and
 * Rupley, J. Mol. Biol. 79 (1973) 351; no counterpart in the reference.  It is the ACC column the secondary-structure section leaves out) ----
 * Per structure of atoms [n, n_res, 5, 3] (atom14 slots N, CA, C, O, CB), with atom_exists [n_res, 5] (bytes, != 0: the atom exists; GLY has
 * no CB) and radii [n_res, 5] float64 (van der Waals radii in Angstrom, the caller's) shared by the n structures.  An atom that does not
 * exist has no surface and buries nothing, whatever its coordinates and its radius.
 *  Expanded radius.  R_a = radii_a + probe, one float64 addition; probe >= 0 is the radius of the solvent sphere (1.4 A for water).
 *  Sphere.  sphere [n_points, 3] float64 unit vectors, built by the HOST and read as they are: no sine or cosine runs on the device, so the
 *     device and a numpy statement of this definition see the same bits.  The binding's table is the golden spiral, for k = 0 .. P - 1:
 *       y = (k (2 / P) - 1) + 1 / P,  r = sqrt(1 - y y),  phi = k (pi (3 - sqrt 5)),  u_k = (cos(phi) r, y, sin(phi) r).
 *  Test point.  p = c_a + R_a u_k per component: the product is rounded, then the sum.  c are the widened float32 coordinates.
 *  Buried.  The point is buried iff some existing atom b != a has (dx dx + dy dy) + dz dz < R_b R_b with d = p - c_b.  Every atom of the
 *     structure counts, those of the point's own residue included.  A comparison with NaN is false.
 *  Outputs.  counts[., r, a] int32 = the points of the atom that are not buried, 0 for an atom that does not exist.
 *     per_residue[., r] float64 in A^2: area_a = (double)count_a w_a with w_a = 4.0 pi R_a R_a / P evaluated left to right (area_a = 0.0 for
 *     an atom that does not exist), summed in slot order (((a0 + a1) + a2) + a3) + a4.
 *     total[.] float64 = the residues' areas, summed in an order that depends on n_res and on the kernel's fixed block shape alone: thread t
 *     of T (512 up to 256 residues, 1024 above) adds the residues t, t + T, ... in ascending order, the 64 lanes of a wave meet in an xor
 *     tree, the waves are added in turn.
 * Arithmetic: everything is float64, one rounding per operation (no contraction).  A wave tests an atom's points only against the atoms
 * with |c_a - c_b|^2 < ((R_a + R_b)(1 + 2^-30) + 2^-30 (1 + M))^2, M = the largest |coordinate| of the structure's existing atoms: an atom
 * that fails cannot bury a point under any rounding (the roundings of the point and of the test are 2^20 times smaller than the slack), so
 * no output depends on this.  A structure's outputs depend on its own coordinates alone: bit for bit the same in any launch.
 * What this is NOT: an all-atom surface.  There are no side chains beyond CB, so absolute values overstate the exposure of large residues,
 * and no relative accessibility against tabulated Gly-X-Gly maxima is formed (no such table is in the tree).  No gradients. */
#define S2S_SASA_MAX_RES 512      /* the structure's atoms stay in LDS as float64 planes with radius and area: 220 B per residue */
#define S2S_SASA_MAX_POINTS 1024  /* the sphere stays in LDS as float64 planes, 24 KiB; a lane of a wave owns 16 points of an atom */

/* No scratch.  n >= 1, 1 <= n_res <= S2S_SASA_MAX_RES, 1 <= n_points <= S2S_SASA_MAX_POINTS, probe finite and >= 0, no NULL buffer;
 * otherwise hipErrorInvalidValue before any launch.  counts [n, n_res, 5] int, per_residue [n, n_res] and total [n] float64. */
int s2s_backbone_sasa(const float* atoms, int n, int n_res, const unsigned char* atom_exists, const double* radii, double probe,
                      const double* sphere, int n_points, int* counts, double* per_residue, double* total, void* stream);

/* ---- Solution scattering: what would a SAXS or a diffusion measurement see of this ensemble?  (csrc/ensemble_saxs.hip; Debye, Ann. Phys.
 * 351 (1915) 809; Kirkwood, J. Polym. Sci. 12 (1954) 1; no counterpart in the reference) ----
 * For a structure of L = n_res CA beads with positions x_i (float32 widened to float64), v_ij = |x_i - x_j|^2 = (dx dx + dy dy) + dz dz,
 * r_ij = sqrt(v_ij), a q-list q_k >= 0 in 1/Angstrom, and a form factor f_i(q_k) = table[types[i], k] (table [n_types, n_q] float64 of any
 * sign: contrast can be negative; types [n_res] int32 in 0 .. n_types - 1; both shared by the n structures):
 *  Intensity (Debye 1915).  I(q_k) = sum_i f_i(q_k)^2 + 2 sum_{i<j} f_i(q_k) f_j(q_k) s(q_k r_ij), with s(a) = 1.0 if a == 0.0, else
 *     sin(a) / a.  One sqrt per pair; one product a = q_k r_ij, one sin and one division per (pair, q); a term is (f_i f_j) s.
 *  Kirkwood hydrodynamic radius.  1 / Rh = (1 / L^2) sum_{i != j} 1 / r_ij.  The kernel returns inv_r_mean = (2 sum_{i<j} 1 / r_ij) / (L L).
 *     L = 1 gives 0 (Rh = inf).  Coincident beads give inf (Rh = 0).
 *  Default form factors (the binding's): one type, all ones.  Every residue is the same point scatterer, so I(0) = L^2.  This is the usual
 *     CA-bead approximation and holds for q <~ 0.3 / Angstrom.
 *  NaN.  A NaN (or infinite) coordinate makes that structure's outputs NaN and touches no other structure: every diagonal term is
 *     f_i^2 + |x_i - x_i|^2, which is f_i^2 for a finite bead, and the same sum of |x_i - x_i|^2 is added to inv_r_mean, so that a
 *     structure of one bead follows the rule as well.
 *  Order of the sums.  A workgroup of 256 threads owns one structure and a tile of 16 consecutive q-values.  Thread t adds the pairs
 *     t, t + 256, ... of the flattened upper triangle (row i holds j = i + 1 .. L - 1) in ascending order, the 64 lanes of a wave meet in
 *     an xor tree, the four waves are added in turn, the diagonal is added in ascending i, then I = diag + 2 off.  The order is a function
 *     of n_res and the block shape alone: a structure's row of intensity and its inv_r_mean are the same bytes in any launch, any chunking,
 *     any position in the batch, and for any q-list that contains the same q at the same offset within its tile.
 * Arithmetic: everything is float64, one rounding per operation (no contraction); sin is the device library's double sine.
 * What this is NOT: there is no hydration shell, no excluded-volume term, no built-in residue form-factor table (the caller brings one),
 * no side chains, and no Nygaard or other correction of the Kirkwood value.  No gradients. */
#define S2S_SAXS_MAX_RES 1024   /* the structure's beads stay in LDS as three float64 planes with their types: 28 KiB */
#define S2S_SAXS_MAX_Q 1024     /* q-values per call, tiles of 16 */
#define S2S_SAXS_MAX_TYPES 64   /* the tile's slice of the table stays in LDS: 8 KiB */

/* No scratch.  n >= 1, 1 <= n_res <= S2S_SAXS_MAX_RES, 1 <= n_q <= S2S_SAXS_MAX_Q, 1 <= n_types <= S2S_SAXS_MAX_TYPES, no NULL buffer but
 * inv_r_mean (NULL: not computed); otherwise hipErrorInvalidValue before any launch.  ca [n, n_res, 3]; intensity [n, n_q] and inv_r_mean
 * [n] float64.  q must be finite and >= 0, the table finite and the types inside the table: the binding checks that before the device. */
int s2s_ca_scattering(const float* ca, int n, int n_res, const double* q, int n_q, const int* types, const double* table, int n_types,
                      double* intensity, double* inv_r_mean, void* stream);

/* ---- Essential dynamics: how does the ensemble move?  Mean structure, covariance and projections of the superposed CA coordinates
 * (csrc/ensemble_pca.hip; what `gmx covar` / `gmx anaeig` compute; no counterpart in the reference) ----
 * x [n, n_res, 3] float32 CA coordinates; xform [n, 12] float64 in s2s_ca_superpose's layout (NULL: the identity); p [n] float64 sample
 * weights, >= 0 and summing to 1 (the caller normalises; NULL: 1 / n each).  With c = 3 i + a the coordinate a of residue i:
 *  Aligned coordinate.  y_sc = ((R_a0 x_i0 + R_a1 x_i1) + R_a2 x_i2) + t_a in float64 on the widened coordinates (contraction allowed: an fma
 *     only removes a rounding); with xform NULL y_sc is the widened x itself.  y is never rounded to float32.
 *  Mean.  m_c = sum_s p_s y_sc.  Thread g of 16 adds the structures g, g + 16, ... in ascending order, the 16 partial sums are added in
 *     ascending g: the order depends on n alone.
 *  Covariance (population form, no Bessel factor; two-pass).  C[r, c] = sum_s p_s (y_sr - m_r)(y_sc - m_c) about the GIVEN mean.  A prepass
 *     writes z_sc = sqrt(p_s) (y_sc - m_c) as float64 into the workspace in blocks of 48 coordinates x 4-padded structures,
 *     ws[(blk * Sp + k) * 48 + r], padding rows and columns zero.  One wave forms a 48 x 48 block of C on v_mfma_f64_16x16x4_f64 in nine
 *     accumulator tiles, the k loop over the structures in ascending order, four per instruction.  Only blocks on or above the diagonal are
 *     computed; every entry with r <= c is stored and copied to (c, r), so C is exactly symmetric.  The structures go through the workspace
 *     in chunks of a multiple of 4; the accumulators of a later chunk start from the running C, so every entry is the same chain of
 *     instructions -- the same bits -- for any workspace size.
 *  Projection.  proj[s, k] = sum_c (y_sc - m_c) v_kc for components v [n_components, 3 n_res] float64.  One wave per structure; lane l adds
 *     the coordinates l, l + 64, ... in ascending order, the lanes meet in the xor tree: the order depends on n_res alone.
 * What this is NOT: an eigensolver (the symmetric eigenproblem of C is the host's), anything beyond CA atoms.  No gradients. */
#define S2S_PCA_MAX_RES 1024   /* 3 n_res = 3072 coordinates: a structure's centred coordinates stay in LDS as float64, 24 KiB */
/* the workspace of s2s_ca_covariance that takes the structures in chunks of `chunk` (rounded up to a multiple of 4) */
#define S2S_PCA_WORKSPACE_DOUBLES(n_res, chunk) ((3ll * (n_res) + 47) / 48 * 48 * (((long long)(chunk) + 3) / 4 * 4))

/* No scratch.  n >= 1, 1 <= n_res <= S2S_PCA_MAX_RES; otherwise hipErrorInvalidValue before any launch.  mean [n_res, 3] float64. */
int s2s_ca_aligned_mean(const float* x, int n, int n_res, const double* xform, const double* p, double* mean, void* stream);

/* cov [3 n_res, 3 n_res] float64, every entry written.  workspace: caller-owned, workspace_doubles >= S2S_PCA_WORKSPACE_DOUBLES(n_res, 4);
 * the chunk is the largest multiple of 4 structures it holds (at most n rounded up to 4).  The same checks.  Per chunk: the prepass, then
 * cov_product_kernel of csrc/ensemble_pca.hip, one wave per 48 x 48 block on or above the diagonal, on the tile set and operands of
 * csrc/sym48_f64.h. */
int s2s_ca_covariance(const float* x, int n, int n_res, const double* xform, const double* p, const double* mean, double* cov,
                      double* workspace, long long workspace_doubles, void* stream);

/* proj [n, n_components] float64.  No scratch.  The same checks, and n_components >= 1. */
int s2s_ca_project(const float* x, int n, int n_res, const double* xform, const double* mean, const double* components, int n_components,
                   double* proj, void* stream);

/* ---- Time-lagged covariances and TICA: which collective coordinates are SLOW?  Reversible mean, instantaneous and time-lagged covariance
 * of a feature trajectory, and projections onto given components (csrc/ensemble_tica.hip; the heavy half of the estimator behind the
 * reference's js_tica, deeptime's Covariance(lagtime, reversible=True, remove_data_mean=True, bessels_correction=False) as oracle/tica.py
 * restates it) ----
 * f [T, D] float32 features, row-major, a row per frame in time order -- ANY features (the CA distances of s2s_ca_pairwise_distances are
 * one choice).  lag >= 1; n = T - lag >= 1 frame pairs (t, t + lag), t = 0 .. n - 1.  Everything is float64 on the widened float32 values;
 * no float atomics.
 *  Mean.  m_c = (1 / 2n) sum_{t<n} (f_tc + f_{t+lag,c}).  Thread g of 16 adds the pairs g, g + 16, ... in ascending order, each as
 *     f_t + f_{t+lag}; the 16 partial sums are added in ascending g, the total is divided by 2n: the order depends on (T, lag) alone.
 *  Covariances (population form, no Bessel factor; two-pass) about the GIVEN mean.  With z_t = (f_t - m) / sqrt(2n):
 *       C00[r, c] = sum_{t<n} (z_tr z_tc + z_{t+lag,r} z_{t+lag,c})        C0t[r, c] = sum_{t<n} (z_tr z_{t+lag,c} + z_{t+lag,r} z_tc)
 *     A prepass writes two operand streams indexed by PAIR, z_t and z_{t+lag} (no halo), as float64 into the workspace in blocks of 48
 *     features x 4-padded pairs, ws[(((s * nblk + blk) * G + g) * step + k) * 48 + r] for stream s, group g, pair slot k; padding features
 *     and padding pairs are zero.  One wave owns a 48 x 48 block with block-row <= block-column and forms BOTH matrices from the same four
 *     operand loads per k-step on v_mfma_f64_16x16x4_f64 (18 accumulator tiles, 36 instructions per 12 loaded doubles per lane), the k
 *     loop over the pairs in ascending order, four per instruction; per step an entry of C00 takes its z_t product, then its z_{t+lag}
 *     product, an entry of C0t its (t, t+lag) product, then its (t+lag, t) product.  Only entries with r <= c are computed; each is stored
 *     and copied to (c, r): both matrices are exactly symmetric.
 *  k-split.  With B = ceil(D / 48) blocks, the triangle has B (B + 1) / 2 of them.  The n pairs, rounded up to a multiple of 4 (n4), are
 *     divided into G contiguous groups of S2S_TICA_GROUP_PAIRS pairs (a multiple of 4; the last group takes what is left):
 *       wanted = max(1, min(S2S_TICA_WAVE_SLOTS / triangle, ceil(n4 / S2S_TICA_MIN_GROUP_PAIRS)))
 *       group  = 4 ceil(n4 / 4 / wanted),   G = ceil(n4 / group)
 *     -- a function of (n, D) alone, never of the workspace.  G = 1 accumulates in C itself.  With G > 1 group g accumulates into partial
 *     blocks of its own in the workspace (the accumulator tiles as the lanes hold them, S2S_TICA_PARTIAL_BLOCK_DOUBLES per block and
 *     matrix); a last kernel adds the partials of an entry in ascending g and writes the entry and its mirror.
 *  Chunking.  The pairs go through the workspace in passes; a pass advances EVERY group by the same number of pairs, a multiple of 4, and
 *     the accumulators of a later pass start from the running values, so every entry is the same chain of instructions -- the same bits
 *     -- for any workspace size.
 *  Projection.  proj[s, k] = sum_c (f_sc - m_c) v_kc for components v [n_components, D] float64.  One wave per row, f read directly (no
 *     staging of the row: D is not bounded by LDS); lane l adds the features l, l + 64, ... in ascending order, the lanes meet in the xor
 *     tree: the order depends on D alone.
 * What this is NOT: an eigensolver (the two symmetric eigenproblems of TICA are the host's), a weighted estimator, a VAMP score.  No
 * gradients. */
#define S2S_TICA_MAX_FEATURES 16384       /* two D x D float64 matrices of 2 GiB each */
#ifndef S2S_TICA_WAVE_SLOTS
#define S2S_TICA_WAVE_SLOTS 1024          /* 256 CUs x 4 SIMDs: one wave of the product kernel per SIMD */
#endif
#define S2S_TICA_MIN_GROUP_PAIRS 512      /* a group is worth a wave from 128 k-steps (4608 MFMAs) on */
#define S2S_TICA_PARTIAL_BLOCK_DOUBLES 2304   /* a 48 x 48 block as 9 accumulator tiles of 64 lanes x 4 registers */
#define S2S_TICA_BLOCKS(D) (((long long)(D) + 47) / 48)
#define S2S_TICA_TRIANGLE(D) (S2S_TICA_BLOCKS(D) * (S2S_TICA_BLOCKS(D) + 1) / 2)
#define S2S_TICA_PAIRS4(T, lag) (((long long)(T) - (long long)(lag) + 3) / 4 * 4)
#define S2S_TICA_MIN_(a, b) ((a) < (b) ? (a) : (b))
#define S2S_TICA_GROUPS_WANTED(D, T, lag)                                                                                        \
    (S2S_TICA_MIN_(S2S_TICA_WAVE_SLOTS / S2S_TICA_TRIANGLE(D), (S2S_TICA_PAIRS4(T, lag) + S2S_TICA_MIN_GROUP_PAIRS - 1) / S2S_TICA_MIN_GROUP_PAIRS) < 1 \
         ? 1                                                                                                                     \
         : S2S_TICA_MIN_(S2S_TICA_WAVE_SLOTS / S2S_TICA_TRIANGLE(D), (S2S_TICA_PAIRS4(T, lag) + S2S_TICA_MIN_GROUP_PAIRS - 1) / S2S_TICA_MIN_GROUP_PAIRS))
#define S2S_TICA_GROUP_PAIRS(D, T, lag) \
    ((S2S_TICA_PAIRS4(T, lag) / 4 + S2S_TICA_GROUPS_WANTED(D, T, lag) - 1) / S2S_TICA_GROUPS_WANTED(D, T, lag) * 4)
#define S2S_TICA_GROUPS(D, T, lag) ((S2S_TICA_PAIRS4(T, lag) + S2S_TICA_GROUP_PAIRS(D, T, lag) - 1) / S2S_TICA_GROUP_PAIRS(D, T, lag))
/* the workspace of s2s_lagged_covariances whose passes advance every group by `chunk` pairs (rounded up to a multiple of 4): the two
 * operand streams of every group, then the partial blocks (none with one group) */
#define S2S_TICA_WORKSPACE_DOUBLES(D, T, lag, chunk)                                                         \
    (2 * S2S_TICA_BLOCKS(D) * 48 * S2S_TICA_GROUPS(D, T, lag) * (((long long)(chunk) + 3) / 4 * 4) +         \
     (S2S_TICA_GROUPS(D, T, lag) > 1 ? S2S_TICA_GROUPS(D, T, lag) * 2 * S2S_TICA_TRIANGLE(D) * S2S_TICA_PARTIAL_BLOCK_DOUBLES : 0))

/* No scratch.  1 <= D <= S2S_TICA_MAX_FEATURES, lag >= 1, lag < T <= 2^31 - 1; otherwise hipErrorInvalidValue before any launch.
 * mean [D] float64. */
int s2s_lagged_mean(const float* f, int T, int D, int lag, double* mean, void* stream);

/* c00, c0t [D, D] float64, every entry written.  workspace: caller-owned, workspace_doubles >= S2S_TICA_WORKSPACE_DOUBLES(D, T, lag, 4); a
 * pass advances every group by the largest multiple of 4 pairs it holds (at most a group's pairs).  The same checks. */
int s2s_lagged_covariances(const float* f, int T, int D, int lag, const double* mean, double* c00, double* c0t, double* workspace,
                           long long workspace_doubles, void* stream);

/* proj [T, n_components] float64.  No scratch.  T >= 1, 1 <= D <= S2S_TICA_MAX_FEATURES, n_components >= 1; otherwise
 * hipErrorInvalidValue before any launch. */
int s2s_feature_project(const float* f, int T, int D, const double* mean, const double* components, int n_components, double* proj,
                        void* stream);

/* ---- PDB text at the exit of the path (HOST pointers, host code; byte-identical to the reference's writers) ---- */

/* protein.to_pdb per model (src/common/protein.py:152-234) over atom37 [n_models, n_res, 37, 3] float32 HOST coordinates with
 * the atom mask of pdb_utils.atom37_to_pdb (src/common/pdb_utils.py:233: sum |xyz| > 1e-7; GLY CB skipped).
 *   aatype / residue_index / chain_index [n_res] int64 or NULL (defaults of protein_with_default_params, pdb_utils.py:175-203:
 *   ALA, 1..n_res, chain 0); b_factors [n_res,37] double or NULL (zeros); MODEL numbers first_model_number + m;
 *   add_end: 0 = none, 1 = an "END" line after every model (to_pdb(add_end=True)), 2 = one bare "END" without newline after
 *   the last model (atom37_to_pdb).  Returns the number of bytes of text; writes them when out != NULL and they fit in
 *   out_capacity (call with out = NULL to size the buffer).  < 0: -1 bad argument / aatype > 20, -2 more than 62 chains. */
long long s2s_format_pdb_models(const float* atom37, int n_models, int n_res, const long long* aatype,
                                const long long* residue_index, const long long* chain_index, const double* b_factors,
                                int first_model_number, int add_end, char* out, long long out_capacity);

/* The same text streamed to a file in bounded blocks of models (append != 0: append to an existing file).
 * Returns bytes written, -3 cannot open, -4 write error. */
long long s2s_write_pdb_models(const char* path, int append, const float* atom37, int n_models, int n_res,
                               const long long* aatype, const long long* residue_index, const long long* chain_index,
                               const double* b_factors, int first_model_number, int add_end);

/* pdb_utils.merge_pdbfiles (src/common/pdb_utils.py:31-83): MODELs of the inputs, in order, renumbered from 1. */
long long s2s_merge_pdb_files(const char* const* paths, int n_paths, const char* out_path);

/* ---- Host noise stream (parity mode) ----
 * Discard n_outputs 32-bit outputs of the Mersenne twister behind torch's CPU generator: state624 = the engine's 624 words in 64-bit
 * slots, *left / *next = its counters, as torch.get_rng_state() serialises them.  The reference draws -- and, under the probability-flow
 * ODE, never uses -- two float64 normal tensors of the whole chunk per denoise step (src/models/score/so3.py:360, src/models/score/r3.py:109);
 * a float64 normal tensor of n >= 16 elements costs 2 (n + (n % 16 ? 16 : 0)) engine outputs, and this call leaves the generator where
 * those draws leave it without computing them (host code; returns 0, or 1 for fields outside the engine's ranges). */
int s2s_mt19937_discard(unsigned long long* state624, int* left, unsigned long long* next, unsigned long long n_outputs);

#ifdef __cplusplus
}
#endif
#endif /* STR2STR_HIP_H */
