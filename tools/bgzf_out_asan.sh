#!/bin/bash
# The BGZF writer under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: tools/bgzf_out_asan.cpp, a program of its own, linked with
# the library sources compiled against the mock HIP runtime, fed the whole corpus of tests/bgzf_out_cases.py.  Nothing is preloaded.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${BWA_AMD_SAN_DIR:-/tmp/bwa_amd_bgzf_out_san}; mkdir -p $OUT
cd $ROOT
python tests/bgzf_out_cases.py --dump $OUT/corpus
g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -x c++ -I $ROOT/tests/hostsim \
    $ROOT/bwa_amd/csrc/bwagpu.hip $ROOT/bwa_amd/csrc/bwagpu_index.hip $ROOT/tests/hostsim/mock_globals.cpp $ROOT/tools/bgzf_out_asan.cpp -o $OUT/bgzf_out_asan -lpthread
ASAN_OPTIONS=detect_leaks=0:detect_stack_use_after_return=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $OUT/bgzf_out_asan $OUT/corpus/*.txt
