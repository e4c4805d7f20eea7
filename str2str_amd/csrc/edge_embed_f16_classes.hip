// s2s_edge_embed_classes_f16x3 (include/str2str_hip.h): the split-f16 edge embedding on the rows of its class table (TABLE), see edge_embed_f16.h.
#include "edge_embed_f16.h"
#include "pair_launch.h"

extern "C" int s2s_edge_embed_classes_f16x3(const float* node_a2, const float* node_b2, const float* rel_table, const float* bin_table,
                                             const void* weight_stream, const float* b2, const float* b3, const float* ln_gamma,
                                             const float* ln_beta, float* table, int n_fixed, int n_rel, int n_bins, float ln_eps,
                                             const float* proj_bias_cat64, int* range_words, void* stream) {
    if (n_fixed < 1 || n_fixed > 2 || n_rel < 1 || n_bins < 1 || n_bins > 32) return (int)hipErrorInvalidValue;
    const long long M = (long long)(n_fixed == 2 ? 4 : 1) * n_rel * (n_bins + 1);   // class rows: every (fa, fb) of the fixed classes present
    if (M * s2s::kEeRecProj * 4 >= (1ll << 32) || (long long)n_rel * 512 >= (1ll << 32)) return (int)hipErrorInvalidValue;   // 32-bit offsets
    const dim3 grid(s2s::persistent_grid(M, s2s::cu_count()));
    if (proj_bias_cat64)
        hipLaunchKernelGGL((edge_embed_f16_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, node_a2, node_b2,
                           rel_table, bin_table, (const float*)nullptr, (const long long*)nullptr, (const float*)nullptr,
                           (const char*)weight_stream, b2, b3, ln_gamma, ln_beta, (const float*)nullptr, table, M, n_fixed, 0, n_rel, n_bins,
                           ln_eps, 0, proj_bias_cat64, (float*)nullptr, (float*)nullptr, range_words);
    else
        hipLaunchKernelGGL((edge_embed_f16_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, node_a2, node_b2,
                           rel_table, bin_table, (const float*)nullptr, (const long long*)nullptr, (const float*)nullptr,
                           (const char*)weight_stream, b2, b3, ln_gamma, ln_beta, (const float*)nullptr, table, M, n_fixed, 0, n_rel, n_bins,
                           ln_eps, 0, (const float*)nullptr, (float*)nullptr, (float*)nullptr, range_words);
    return (int)hipGetLastError();
}
