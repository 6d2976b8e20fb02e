#!/bin/bash
# Build tests/host/msda_grid_host_check.cpp (csrc/msda_grid.h, the region-grid chooser, with the knobs of csrc/msda_tuning.h) for the
# host and run it.
#   tools/msda_grid_host_check.sh              under AddressSanitizer + UBSan: the form to run by hand on a CPU machine after a
#                                              change to msda_grid.h (a sanitizer run does not belong on a GPU machine)
#   CXXFLAGS= tools/msda_grid_host_check.sh    a plain build: what tests/test_msda_grid_host.py runs with the suite, anywhere
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
D=$(mktemp -d)
trap 'rm -rf "$D"' EXIT
${CXX:-g++} -std=c++17 -O1 -g -Wall ${CXXFLAGS--fsanitize=address,undefined -fno-sanitize-recover=all} \
    -I"$R/semi-detr_amd/csrc" "$R/tests/host/msda_grid_host_check.cpp" -o "$D/msda_grid_host_check" -pthread
"$D/msda_grid_host_check"
