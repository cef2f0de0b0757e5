#!/bin/bash
# CPU-only sanitizer pass (ASan + UBSan) over the host generators and the oracle, and over the host planners (tb_planners.cpp, tb_spmv_planners.cpp) through
# tests/planner_driver.cpp on the meshes of tests/test_planners_cpu.py.  Stand-alone programs, run directly.
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../.." && pwd); csrc="$root/thunderbolt.jl_amd/csrc"
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
san="-g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -fopenmp -D__HIP_PLATFORM_AMD__ -I$root/include -I/opt/rocm/include -I$root/oracle -I$csrc"
pids=()
for src in "$here/host_driver.cpp" "$csrc/tb_hostgen.cpp" "$root/tests/planner_driver.cpp" "$csrc/tb_planners.cpp" "$csrc/tb_spmv_planners.cpp"; do
    g++ -std=c++17 $san -c "$src" -o "$out/$(basename "$src" .cpp).o" & pids+=($!)
done
gcc $san -c "$root/oracle/tb_oracle.c" -o "$out/tb_oracle.o" & pids+=($!)
for pid in "${pids[@]}"; do wait "$pid"; done
g++ $san "$out/host_driver.o" "$out/tb_hostgen.o" "$out/tb_oracle.o" -lm -o "$out/drv"
g++ $san "$out/planner_driver.o" "$out/tb_planners.o" "$out/tb_spmv_planners.o" "$out/tb_hostgen.o" -o "$out/planner_driver"
export ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1
"$out/drv"
meshes=$1 # a directory of meshes as tests/test_planners_cpu.py writes them; without one they are written here, which needs the built library
if [ -z "$meshes" ]; then
    meshes="$out/meshes"; mkdir "$meshes"
    (cd "$root/tests" && python3 -c "import sys; sys.path.insert(0, '..'); import thunderbolt_jl_amd as tb, test_planners_cpu as t; t.write_meshes(tb, sys.argv[1])" "$meshes")
fi
for threads in 1 4; do OMP_NUM_THREADS=$threads "$out/planner_driver" "$meshes" > /dev/null; done
echo "planners clean"
