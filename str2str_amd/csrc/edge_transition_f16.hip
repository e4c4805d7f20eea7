// s2s_edge_transition_f16x3 (include/str2str_hip.h): the public entry point, and the edge transition for chains of 32+ residues
// (STAGE: the tile's row seeds go through LDS).  The two other forms are units of their own, see edge_transition_f16.h.
#include "edge_transition_f16.h"

extern "C" int s2s_edge_transition_f16x3(const float* edge, const float* node_ab, const float* node_p, const void* weight_stream,
                                          const float* b2, const float* ln_gamma, const float* ln_beta, const float* mask, float* out,
                                          int n_samples, int n_res, float ln_eps, int io_layout, const float* proj_bias_cat64,
                                          float* proj_attn_bias, float* proj_pair_z, int prescale_exp, int* range_words, void* stream) {
    const s2s::EtArgs a = {edge, node_ab, node_p, weight_stream, b2, ln_gamma, ln_beta, mask, out, n_samples, n_res, ln_eps, io_layout,
                           proj_bias_cat64, proj_attn_bias, proj_pair_z, prescale_exp, range_words, stream};
    if (io_layout & 8) return s2s::et_f16x3_by_class(a);
    return n_res >= 32 ? et_launch<true>(a) : s2s::et_f16x3_short_chains(a);
}
