#!/bin/bash
# Build tests/host/msda_exactsum_host_check.cpp (csrc/msda_exactsum.h alone, no HIP) for the host and run it on stdin.
#   tools/msda_exactsum_host_check.sh              under AddressSanitizer + UBSan: the form to run by hand on a CPU machine after
#                                                  a change to msda_exactsum.h (a sanitizer run does not belong on a GPU machine)
#   CXXFLAGS= tools/msda_exactsum_host_check.sh    a plain build: what tests/test_msda_exact_ref.py runs with the suite, anywhere
# Requests on stdin, one per line (see the program's header); e.g.  echo "S 3f800000 bf800000 00000001" | tools/msda_exactsum_host_check.sh
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
${CXX:-g++} -std=c++17 -O1 -g ${CXXFLAGS--fsanitize=address,undefined -fno-sanitize-recover=all} \
    -I"$R/semi-detr_amd/csrc" "$R/tests/host/msda_exactsum_host_check.cpp" -o "$D/msda_exactsum_host_check"
"$D/msda_exactsum_host_check"
