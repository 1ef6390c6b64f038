#!/bin/bash
# builds the SZ4_DIAG=N variant of the HIP library (3: per-wavefront counters of k_find_sorted, 5: k_find_long9,
# 6: k_find_big's phase clocks, 7: k_dp_fix's repair) as smallz4_amd/lib/libsmallz4_amd_diagN.so
exec make -C "$(dirname "$0")/../smallz4_amd/csrc" OUT=../lib/libsmallz4_amd_diag${1:-3}.so EXTRA="-DSZ4_DIAG=${1:-3}" ../lib/libsmallz4_amd_diag${1:-3}.so
