// s2s_edge_embed_f16x3 (include/str2str_hip.h): the split-f16 edge embedding on pairs, see edge_embed_f16.h.
#include "edge_embed_f16.h"
#include "pair_launch.h"

extern "C" int s2s_edge_embed_f16x3(const float* node_a, const float* node_b, const float* rel_table, const float* bin_table,
                                     const float* bin_lower, const long long* residue_idx, const float* ca_xyz,
                                     const void* weight_stream, const float* b2, const float* b3, const float* ln_gamma,
                                     const float* ln_beta, const float* mask, float* out, int n_samples, int n_res,
                                     int rel_offset, int n_rel, int n_bins, float ln_eps, int out_tiled, const float* proj_bias_cat64,
                                     float* proj_attn_bias, float* proj_pair_z, int* range_words, void* stream) {
    if (n_samples <= 0 || n_res <= 0) return 0;
    if (n_bins > 32 || (out_tiled & ~1)) return (int)hipErrorInvalidValue;  // the distogram edges are counted from a 32-entry LDS table
    // 32-bit pair indices and buffer offsets inside a launch: split the samples over several launches when needed
    const long long NN = (long long)n_res * n_res;
    if (NN >= (1ll << 31) || (long long)n_rel * 512 >= (1ll << 32)) return (int)hipErrorInvalidValue;
    const long long rows_cap = ((1ll << 32) - 1) / ((long long)n_res * 512);  // node_b descriptor
    const long long chunk = s2s::samples_per_launch("S2S_EE_MAX_PAIRS", (1ll << 31) - 1, NN, n_samples, out_tiled != 0, rows_cap);
    if (chunk < 1) return (int)hipErrorInvalidValue;
    const int n_cu = s2s::cu_count();
    for (long long b0 = 0; b0 < n_samples; b0 += chunk) {
        const long long nb = n_samples - b0 < chunk ? n_samples - b0 : chunk;
        const long long M = nb * NN, rows0 = b0 * n_res;
        const dim3 grid(s2s::persistent_grid(M, n_cu));
        const float* na = node_a + rows0 * 128;
        const float* nbp = node_b + rows0 * 128;
        const long long* ridx = residue_idx + rows0;
        const float* cap = ca_xyz + rows0 * 3;
        const float* mk = mask ? mask + rows0 : nullptr;
        float* o = out + b0 * NN * 128;
        if (proj_attn_bias)
            hipLaunchKernelGGL(edge_embed_f16_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, na, nbp,
                               rel_table, bin_table, bin_lower, ridx, cap, (const char*)weight_stream, b2, b3, ln_gamma, ln_beta,
                               mk, o, M, n_res, rel_offset, n_rel, n_bins, ln_eps, out_tiled, proj_bias_cat64,
                               proj_attn_bias + b0 * 8 * NN, proj_pair_z + b0 * NN * 32, range_words);
        else
            hipLaunchKernelGGL(edge_embed_f16_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, na, nbp,
                               rel_table, bin_table, bin_lower, ridx, cap, (const char*)weight_stream, b2, b3, ln_gamma, ln_beta,
                               mk, o, M, n_res, rel_offset, n_rel, n_bins, ln_eps, out_tiled, (const float*)nullptr, (float*)nullptr,
                               (float*)nullptr, range_words);
    }
    return (int)hipGetLastError();
}
