#!/bin/bash
# Diagnostic builds of libsdfnmpc.so with extra defines into _build/<name>/ (never the product library):
#   tools/build_variant.sh nomfma -DSDF_NO_MFMA
# It is the product Makefile with its object and library directories redirected and the extra flags appended to
# the product's own, so it compiles whatever the product compiles, each kernel file with the product's per-file
# flags (FLAGS_* there): -amdgpu-mfma-vgpr-form goes to rti_qp, vae_enc and sdf_wide only, not to every kernel file.
set -euo pipefail
name=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
O=$R/_build/$name
extra=$(printf '%q ' "$@")  # quoted once more for the recipe's shell: a -D value may hold spaces
make -s -j"${MAX_JOBS:-16}" -C "$R/sdf-nmpc_amd/csrc" OBJ="$O" LIBDIR="$O" EXTRA_CXXFLAGS="$extra" "$O/libsdfnmpc.so"
echo "$O/libsdfnmpc.so"
