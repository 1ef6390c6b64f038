#!/bin/bash
# builds a tuning variant of the HIP library: tools/build_variant.sh NAME "-DSZ4_X=..." -> lib/libsmallz4_amd_NAME.so
# (select it with SMALLZ4_AMD_LIB=smallz4_amd/lib/libsmallz4_amd_NAME.so)
exec make -C "$(dirname "$0")/../smallz4_amd/csrc" OUT=../lib/libsmallz4_amd_$1.so EXTRA="$2" ../lib/libsmallz4_amd_$1.so
