#!/bin/bash
# Build tests/host/common_host_check.cpp (csrc/common.cpp with the two HIP calls stubbed) for the host and run it.
#   tools/common_host_check.sh              under AddressSanitizer + UBSan: the form to run by hand on a CPU machine after a
#                                           change to common.cpp / common.h (a sanitizer run does not belong on a GPU machine)
#   CXXFLAGS= tools/common_host_check.sh    a plain build: what tests/test_common_host.py runs with the suite, anywhere
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
${CXX:-g++} -std=c++17 -O1 -g ${CXXFLAGS--fsanitize=address,undefined -fno-sanitize-recover=all} -D__HIP_PLATFORM_AMD__=1 \
    -I"$R/semi-detr_amd/csrc" -I"$R/include" -I"${ROCM_PATH:-/opt/rocm}/include" \
    "$R/tests/host/common_host_check.cpp" "$R/semi-detr_amd/csrc/common.cpp" -o "$D/common_host_check"
"$D/common_host_check"
