#!/bin/bash
# A second libdrx built with extra compiler flags, for A/B runs on one box:
#   bash scripts/build_variant.sh <name> "<flags>"   ->  drecpy_amd/csrc/build/libdrx_<name>.so
#   DRX_HOST_SANITIZER_LIB=drecpy_amd/csrc/build/libdrx_<name>.so python bench.py ...     (drecpy_amd/_lib.py loads that file instead)
set -eu
NAME=$1; FLAGS=${2:-}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OBJ=$ROOT/drecpy_amd/csrc/build/var_$NAME
mkdir -p $OBJ
# the source list is the library's own (drecpy_amd/build.py SOURCES): .hip with hipcc, .cpp with g++, as there
SRCS=$(python3 -c "import runpy, sys; print(' '.join(runpy.run_path(sys.argv[1])['SOURCES']))" $ROOT/drecpy_amd/build.py)
pids=""
for s in $SRCS; do
  case $s in
    *.hip) /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -I $ROOT/include -I $ROOT/drecpy_amd/csrc $FLAGS -c $ROOT/drecpy_amd/csrc/$s -o $OBJ/$s.o & ;;
    *)     g++ -pthread -O3 -fPIC -std=c++17 -I $ROOT/include -I $ROOT/drecpy_amd/csrc -c $ROOT/drecpy_amd/csrc/$s -o $OBJ/$s.o & ;;
  esac
  pids="$pids $!"
done
for p in $pids; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $ROOT/drecpy_amd/csrc/build/libdrx_$NAME.so $(for s in $SRCS; do echo $OBJ/$s.o; done) -ldl
echo $ROOT/drecpy_amd/csrc/build/libdrx_$NAME.so
