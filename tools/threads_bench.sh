#!/bin/bash
# T host threads of single granne_hip_search calls, GRANNE_HIP_OPT_COALESCE off and on (tools/threads_bench.cpp):
#   bash tools/threads_bench.sh [--seconds 2 --threads 1,4,16 --rounds 3 --elements 1000000 --out profiles/coalesce_threads.json]
# Builds the library and the program where they are missing or stale, then runs the program under ONE time limit
# (THREADS_BENCH_TIMEOUT seconds, default 540); the program stops at the first non-zero status.
set -euo pipefail
cd "$(dirname "$0")/.."
LIB_DIR=$PWD/granne_amd/lib
python -m granne_amd.build >/dev/null
if [ ! -x tools/threads_bench ] || [ tools/threads_bench.cpp -nt tools/threads_bench ] || [ include/granne.hpp -nt tools/threads_bench ]; then
  g++ -std=c++17 -O2 -Wall -pthread -I include tools/threads_bench.cpp -L "$LIB_DIR" -lgranne_hip \
      -Wl,-rpath,'$ORIGIN/../granne_amd/lib' -Wl,--allow-shlib-undefined -o tools/threads_bench
fi
export LD_LIBRARY_PATH=/opt/rocm/lib:${LD_LIBRARY_PATH:-}
exec timeout -k 10 "${THREADS_BENCH_TIMEOUT:-540}" tools/threads_bench "$@"
