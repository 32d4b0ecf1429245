#!/bin/bash
# Build an A/B variant of libshdtopo.so with extra compile-time defines (kernel experiments).
#   tools/build_variant.sh NAME -DSHD_BATCH_RB=3 ...   ->  abtest/NAME/libshdtopo.so
# Load it with SHDTOPO_LIB=abtest/NAME/libshdtopo.so (shadow_amd/_lib.py); time it on the GPU box
# with tools/ab_probe.sh.  The sources and flags are the Makefile's.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1
shift
OUT=$ROOT/abtest/$NAME
make -s -j"$(nproc | awk '{print ($1 < 16) ? $1 : 16}')" -C "$ROOT/shadow_amd/csrc" \
  OBJDIR="$OUT/obj" OUT="$OUT" EXTRAFLAGS="$*" "$OUT/libshdtopo.so"
echo "$OUT/libshdtopo.so"
