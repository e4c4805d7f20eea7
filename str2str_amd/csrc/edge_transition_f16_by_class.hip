// The split-f16 edge transition reading its edge rows BY CLASS (io_layout bit 3), see edge_transition_f16.h.
#include "edge_transition_f16.h"

int s2s::et_f16x3_by_class(const EtArgs& a) {
    // the records (zero record + class rows) are addressed with 32-bit byte offsets: below 4 GB is the caller's contract (header), it
    // cannot be checked here -- the row count is no argument of this entry point
    return a.n_res >= 32 ? et_launch<true, true>(a) : et_launch<false, true>(a);
}
