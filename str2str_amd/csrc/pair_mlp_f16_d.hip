// Translation unit 4 of pair_mlp_f16.hip: the edge embedding on the rows of its class table; see S2S_PM_PART there.
#define S2S_PM_PART 4
#include "pair_mlp_f16.hip"
