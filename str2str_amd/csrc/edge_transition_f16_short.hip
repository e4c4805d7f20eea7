// The split-f16 edge transition for chains below 32 residues (row seeds as per-lane loads), see edge_transition_f16.h.
#include "edge_transition_f16.h"

int s2s::et_f16x3_short_chains(const EtArgs& a) { return et_launch<false>(a); }
