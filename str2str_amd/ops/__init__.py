"""Python binding of libstr2str_hip.so (include/str2str_hip.h) over ctypes, one module per concern.

torch is plumbing here: it owns device memory and the current HIP stream; every op hands raw device pointers + sizes + the stream to
one C-ABI entry point.  There is NO fallback: if the library is missing or a tensor is not a contiguous float32 CUDA(HIP) tensor the
op raises.  The ops are also registered as ``torch.ops.str2str_amd.*`` custom ops (torch_ops.py), at the bottom of this module.
The names below are the objects of the submodules themselves; module state that is rebound (the library handle, the host-RNG
verdict, the registration flag) stays in its module and is reached through that module's functions."""
from .attention import encoder_attention, ipa_attention, ipa_attention_f16, ipa_prep_points, ipa_prep_points_f16
from .binding import (ABI_VERSION, EXPORTS, KINETICS_ABI_VERSION, KINETICS_EXPORTS, LIB_PATH, HipLibraryError, KernelTimer, WeightRangeError,
                      load_library)
from .ensemble import (CLUSTER_MAX_N, CONTACT_MAX_RES, LDDT_MAX_RES, PCA_MAX_RES, RMSD_LAUNCH_PAIRS, SASA_MAX_POINTS, SASA_MAX_RES, SAXS_MAX_Q, SAXS_MAX_RES,
                       SAXS_MAX_TYPES, SS_MAX_RES, TM_MAX_RES, VIOL_MAX_RES, apply_xform, backbone_sasa, backbone_violations, ca_aligned_mean, ca_contact_map, ca_covariance, ca_fit_transforms, ca_project, ca_contact_stats, ca_lddt_matrix, ca_native_contacts, ca_native_q, ca_lddt_per_residue, ca_pairwise_distances, ca_pwd_js, ca_rmsd_matrix,
                       ca_sample_stats, ca_scattering, ca_superpose, ca_tm_matrix, ca_tm_superpose, cluster_adjacency, cluster_gromos,
                       lddt_workspace_bytes, rmsd_row_chunk, secondary_structure, sphere_points,
                       TICA_MAX_FEATURES, feature_project, lagged_covariances, lagged_mean, tica_groups)
from .kinetics import KINETICS_MAX_CENTRES, KINETICS_MAX_DIM, farthest_points, kmeans_assign, kmeans_update, transition_counts
from .geometry import forward_marginal, frames_to_backbone, rigid_compose_update, rigid_scale_trans, se3_step, torsion_head
from .hostio import (float64_normal_outputs, format_pdb_models, host_rng_can_discard, host_rng_discard_float64_normals,
                     host_rng_fast_forward_ok, merge_pdb_files, write_pdb_models)
from .node import (CHAIN_WIDTHS, NARROW_MAX_WORK, SMALL_ROWS, embed_assemble, ipa_projections, node_apply,
                   node_apply_chain, node_apply_multi, node_chain, node_linear, node_linear_f32, node_linear_multi, node_linear_vfrag,
                   pack_planes, row_layernorm, small_rows_variant, to_act)
from .packing import (NODE_TG, LazyDict, PairByClass, PairTiled, act_alloc, column_blocked, fragment_order, node_tiles, pack_f16x2_layer, pack_f16x3_embed_stream,
                      pack_f16x3_stream, pack_node_layer, pack_node_weight, pack_node_weight_f32, pack_weight, padded_len, pair_tiled,
                      pair_untiled, unpack_planes, vf_alloc, xp_alloc)
from .pair import (EE_CLASS_R, edge_embed, edge_embed_class_of_row, edge_embed_class_row, edge_embed_class_rows, edge_embed_classes_eligible,
                   edge_embed_classes_f16x3, edge_embed_f16x3, edge_transition, edge_transition_f16x3, pair_project)
from .range_guard import (RANGE_BITS, RANGE_FAMILIES, range_families, range_flag, range_flag_names, range_flag_read, range_flag_reset,
                          range_headroom)
from .torch_ops import register_torch_ops

__all__ = [
    "ABI_VERSION", "EXPORTS", "LIB_PATH", "HipLibraryError", "KernelTimer", "WeightRangeError", "load_library",
    "RANGE_BITS", "RANGE_FAMILIES", "range_families", "range_flag", "range_flag_names", "range_flag_read", "range_flag_reset", "range_headroom",
    "NODE_TG", "LazyDict", "PairByClass", "PairTiled", "act_alloc", "column_blocked", "fragment_order", "node_tiles", "pack_f16x2_layer", "pack_f16x3_embed_stream",
    "pack_f16x3_stream", "pack_node_layer", "pack_node_weight", "pack_node_weight_f32", "pack_weight", "padded_len", "pair_tiled", "pair_untiled",
    "unpack_planes", "vf_alloc", "xp_alloc",
    "edge_embed", "edge_embed_f16x3", "edge_transition", "edge_transition_f16x3", "pair_project",
    "EE_CLASS_R", "edge_embed_class_of_row", "edge_embed_class_row", "edge_embed_class_rows", "edge_embed_classes_eligible", "edge_embed_classes_f16x3",
    "encoder_attention", "ipa_attention", "ipa_attention_f16", "ipa_prep_points", "ipa_prep_points_f16",
    "CHAIN_WIDTHS", "NARROW_MAX_WORK", "SMALL_ROWS", "embed_assemble", "ipa_projections", "node_apply",
    "node_apply_chain", "node_apply_multi", "node_chain", "node_linear", "node_linear_f32", "node_linear_multi", "node_linear_vfrag", "pack_planes",
    "row_layernorm", "small_rows_variant", "to_act",
    "forward_marginal", "frames_to_backbone", "rigid_compose_update", "rigid_scale_trans", "se3_step", "torsion_head",
    "RMSD_LAUNCH_PAIRS", "apply_xform", "ca_pairwise_distances", "ca_pwd_js", "ca_rmsd_matrix", "ca_sample_stats", "ca_superpose", "rmsd_row_chunk",
    "TM_MAX_RES", "ca_tm_matrix", "ca_tm_superpose",
    "LDDT_MAX_RES", "ca_lddt_matrix", "ca_lddt_per_residue", "lddt_workspace_bytes",
    "VIOL_MAX_RES", "backbone_violations",
    "SS_MAX_RES", "secondary_structure",
    "SASA_MAX_POINTS", "SASA_MAX_RES", "backbone_sasa", "sphere_points",
    "SAXS_MAX_Q", "SAXS_MAX_RES", "SAXS_MAX_TYPES", "ca_scattering",
    "CONTACT_MAX_RES", "ca_contact_map", "ca_contact_stats", "ca_native_contacts", "ca_native_q",
    "PCA_MAX_RES", "ca_aligned_mean", "ca_covariance", "ca_fit_transforms", "ca_project",
    "TICA_MAX_FEATURES", "feature_project", "lagged_covariances", "lagged_mean", "tica_groups",
    "CLUSTER_MAX_N", "cluster_adjacency", "cluster_gromos",
    "KINETICS_ABI_VERSION", "KINETICS_EXPORTS", "KINETICS_MAX_CENTRES", "KINETICS_MAX_DIM", "farthest_points", "kmeans_assign", "kmeans_update",
    "transition_counts",
    "float64_normal_outputs", "format_pdb_models", "host_rng_can_discard", "host_rng_discard_float64_normals", "host_rng_fast_forward_ok",
    "merge_pdb_files", "write_pdb_models",
    "register_torch_ops",
]

register_torch_ops()
