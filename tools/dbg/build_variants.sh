#!/bin/bash
# instrumentation variants of the library (never shipped): tools/dbg/libhsr_<name>.so, selected with HSR_LIBRARY=...
#   tools/dbg/build_variants.sh "name:-DHSR_PHASE_STAMPS[:source]" ...   (source defaults to hsr_srf)
#   tools/dbg/build_variants.sh "gstamp:-DHSR_GRAM_STAMPS:hsr_gram"       (the Gram timeline of tools/gram_stamps.py)
# The sources and the flags are the Makefile's own (its `variant` target): there is no second list here to fall behind.
set -e
cd "$(dirname "$0")/../../hyperspectral_super-resolution_amd/csrc"
for v in "$@"; do
  IFS=: read -r name defs src <<< "$v"
  make variant NAME="$name" DEFS="$defs" ${src:+SRC="$src"}
  echo built $name
done
