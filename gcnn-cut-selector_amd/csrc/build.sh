#!/bin/sh
# Build libgcnn_hip.so for MI355X (gfx950).  hipcc cross-compiles without a GPU.
# `build.sh tuning`: the experiment build libgcnn_hip_tuning.so instead -- the same sources with -DGCNN_TUNING, which reads the
# tuning knobs of tools/README.md from the environment (the variant tests force each dispatch variant through it).
# `build.sh plain`: libgcnn_hip_plain.so -- the same sources with -DGCNN_STORE_PLAIN, every write-through result store (store16,
# gcnn_common.hpp) as a plain one: the reference tests/test_gpu_write_through.py compares the product's stores against.
set -e
cd "$(dirname "$0")"
if [ "$1" = tuning ]; then
  shift
  exec /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -shared -fPIC -DGCNN_TUNING -o libgcnn_hip_tuning.so gcnn_capi.hip "$@"
fi
if [ "$1" = plain ]; then
  shift
  exec /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -shared -fPIC -DGCNN_STORE_PLAIN -o libgcnn_hip_plain.so gcnn_capi.hip "$@"
fi
exec /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -shared -fPIC -o libgcnn_hip.so gcnn_capi.hip "$@"
