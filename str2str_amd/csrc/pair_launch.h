// Host side of the pair-stream launches (edge transition, edge embedding, class-table expansion).  A kernel of the pair stream indexes
// its pairs with 32 bits, so an entry point splits its samples over several launches when needed: this is the one statement of that split.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>

namespace s2s {

// smallest number of samples whose pairs fill whole 32-pair blocks (launch boundaries of a tiled pair tensor)
inline long long tile_aligned_samples(long long NN) {
    long long q = 32;
    while (q > 1 && (NN * (32 / q)) % 32 != 0) q /= 2;   // 32 / q samples suffice when NN (32 / q) is a multiple of 32
    return 32 / q;
}

// persistent workgroups: one per CU of the current device
inline int cu_count() {
    int dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)
        return 256;
    return n_cu;
}
// ... each walking the 128-pair tiles of M pairs
inline unsigned persistent_grid(long long M, int n_cu) { return (unsigned)((M + 127) / 128 < n_cu ? (M + 127) / 128 : n_cu); }

// -> samples per launch, or 0 where not even one sample fits (the caller returns hipErrorInvalidValue).
// hook_env: the test hook, read on every call: a smaller per-launch pair budget exercises the split (<= 0 or above the hard cap: the hard
// cap).  NN: pairs per sample.  tiled: launches of a tiled tensor start on a 32-pair block.  max_samples: a further bound of the caller's.
inline long long samples_per_launch(const char* hook_env, long long hard_cap_pairs, long long NN, int n_samples, bool tiled,
                                    long long max_samples = LLONG_MAX) {
    const char* cap_env = getenv(hook_env);
    long long cap = cap_env ? atoll(cap_env) : 0;
    if (cap <= 0 || cap > hard_cap_pairs) cap = hard_cap_pairs;
    long long chunk = cap / NN < max_samples ? cap / NN : max_samples;
    if (tiled && chunk < n_samples) chunk -= chunk % tile_aligned_samples(NN);
    return chunk < 1 ? 0 : chunk;
}

}  // namespace s2s
