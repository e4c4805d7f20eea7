// Translation unit 5 of pair_mlp_f16.hip: the edge transition reading its edge rows by class; see S2S_PM_PART there.
#define S2S_PM_PART 5
#include "pair_mlp_f16.hip"
