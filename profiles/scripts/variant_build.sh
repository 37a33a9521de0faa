#!/bin/bash
# profiles/scripts/variant_build.sh TU NAME "EXTRA FLAGS": compile ONE translation unit of cddp-cpp_amd/csrc with extra flags and link it
# with the other objects of the product build (run `make` there first) into a separate library scratch/libs/libNAME.so, selected at
# run time with CDDP_HIP_LIB.  The library has no compile-time kernel variants (profiles/design_history.md, "compile-time experiments
# retired"); this builds the timing libraries:
#   variant_build.sh stacks sc_time "-DSC_TIMING"                     (profiles/scripts/sc_times.py)
#   variant_build.sh inst_cartpole roles_time "-DCDDP_ROLES_TIMING"   (profiles/scripts/roles_times.py)
#   variant_build.sh inst_cartpole k4_time "-DCDDP_K4_TIMING"         (profiles/scripts/k4_block_times.py)
#   variant_build.sh inst_terminal te_time "-DTE_EXP=9"               (profiles/scripts/te_phase_timers.py)
set -e
repo=$(cd "$(dirname "$0")/../.." && pwd)
cd $repo/cddp-cpp_amd/csrc
tu=$1; name=$2; extra=$3
HIPCC=${HIPCC:-hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -ffp-contract=off -fno-signed-zeros -DCDDP_TRIG_SHARED=1 $extra"
mkdir -p $repo/scratch/objs $repo/scratch/libs
$HIPCC $FLAGS -c $tu.hip -o $repo/scratch/objs/${tu}_$name.o || { echo FAILED $name; exit 1; }
objs=$(ls ../build/*.o | grep -v "/$tu.o")
$HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,-Bsymbolic -o $repo/scratch/libs/lib$name.so $objs $repo/scratch/objs/${tu}_$name.o -ldl && echo LINKED $name
