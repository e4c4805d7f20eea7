#!/bin/bash
# tools/build_variant.sh <name> [extra hipcc flags]: library variant with one differently compiled unit
# (UNIT=edge_transition_f16 by default = the edge transition for chains of 32+ residues; UNIT=edge_transition_f16_short its short-chain form,
# UNIT=edge_transition_f16_by_class its by-class form, UNIT=edge_embed_f16 / edge_embed_f16_classes the edge embedding; SRC=<file> names another
# version of that one unit, e.g. git show <rev>:str2str_amd/csrc/ipa_attention.hip > old.hip; UNIT=ipa_attention SRC=old.hip tools/build_variant.sh old).  Run
# `python -m str2str_amd.build` first: the other units are linked from its objects.
# NOTE: .gpurunignore lists str2str_amd/csrc/build/ab_*.so (45 stale variants once cost every lease a 73 MB push): comment that line out for an
# A/B session and delete the variants afterwards (rm str2str_amd/csrc/build/ab_*.so).
N=$1; shift
U=${UNIT:-edge_transition_f16}
D=str2str_amd/csrc/build
# the unit's own flags come from str2str_amd/build.py (e.g. -fno-slp-vectorize of the MFMA units: a variant built without them is not comparable)
FLAGS=$(python -c "from str2str_amd.build import UNITS, COMMON; print(' '.join(COMMON + UNITS['$U.hip']))")
SRC=${SRC:-str2str_amd/csrc/$U.hip}     # SRC=<file>: another version of the unit's source (e.g. from git show)
hipcc -x hip -c $SRC -o $D/${U}_$N.o $FLAGS -w "$@" || exit 1
OBJS=""
for u in $(python -c "from str2str_amd.build import UNITS; print(' '.join(k.rsplit('.',1)[0] for k in UNITS))"); do
  if [ $u == $U ]; then OBJS="$OBJS $D/${U}_$N.o"; else OBJS="$OBJS $D/$u.o"; fi
done
hipcc -shared -fPIC --offload-arch=gfx950 -o $D/ab_$N.so $OBJS && echo $D/ab_$N.so
