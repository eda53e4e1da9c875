#!/bin/bash
# A variant library for A/B runs (K4_LIB=4k-nerf_amd/lib4k_hip_<tag>.so): the product's sources, every one compiled with the extra -D flags.
# usage: bash tools/build_variant.sh <tag> -DFLAG=VALUE ...      (build container; the .so travels to the GPU box with the snapshot)
# The flag line lives in build.py alone; this is `python 4k-nerf_amd/build.py --tag <tag> -DFLAG=VALUE ...`.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
TAG=$1; shift
exec python "$R/4k-nerf_amd/build.py" --tag "$TAG" "$@"
