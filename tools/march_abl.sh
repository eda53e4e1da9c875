#!/bin/bash
# ablations of the shading kernel (WRONG results, timing only): bash tools/march_abl.sh [K4_DEBUG bits ...]   (GPU box)
# The ablation bits exist only in a -DK4_ABLATE library (csrc/k4_env.h); the default library ignores them.  Build it first, where the compiler is.
R=$(cd "$(dirname "$0")/.." && pwd)
cd $R
ABL=$R/4k-nerf_amd/lib4k_hip_ablate.so
if [ ! -f "$ABL" ]; then
  echo "tools/march_abl.sh: $ABL is missing; build it with:  python 4k-nerf_amd/build.py --tag ablate -DK4_ABLATE" >&2
  exit 1
fi
for dbg in ${@:-0 1 2 512}; do echo "== K4_DEBUG=$dbg"; bash tools/march_prof.sh abl_$dbg K4_LIB=$ABL K4_DEBUG=$dbg 2>&1 | grep -E "shade|geom3|isolated" | awk -F, '{ if (NF>=4) printf "   %-60s %9.1f us\n", substr($1,1,60), $4/1000; else print }'; done
