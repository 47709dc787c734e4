#!/bin/bash
# Diagnostic variants of the scan side (scan.hip -DKPE_DIAG=<bits>): the WIDE general scan
# without its rule evaluation (1), term evaluation (2) or label fold (4), linked with the build's
# other objects into kyverno_amd/build/var/libkpe_d<bits>.so (KPE_LIB selects
# one). Needs a finished `make -C kyverno_amd`.
# Usage: scripts/diag_scan.sh 1 3 7 ...
set -e
cd "$(dirname "$0")/../kyverno_amd"
ROCM=${ROCM:-/opt/rocm}
mkdir -p build/var
OTHERS=$(printf 'build/%s.o ' flatten program synth pss_msg rhash report kpe_api api_results results pssx pattern pattern_trace cond cond_fepat)
for d in "$@"; do
  $ROCM/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-result -munsafe-fp-atomics -fno-vectorize \
    -fno-slp-vectorize -DKPE_DIAG=$d -c csrc/scan.hip -o build/var/scan_d$d.o
  $ROCM/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o build/var/libkpe_d$d.so $OTHERS build/var/scan_d$d.o -lpthread
  echo "built build/var/libkpe_d$d.so"
done
