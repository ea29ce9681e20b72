#!/bin/bash
# Debug build with per-stage timestamps in the fit kernel -> m-loam_amd/lib/libmloam_hip_dbg.so (not the product library)
set -e
cd "$(dirname "$0")/../m-loam_amd/csrc"
mkdir -p ../lib/dbg
# (every translation unit of the product library: m-loam_amd/build.py's SOURCES)
SOURCES=$(python3 -c "import importlib.util as u; s = u.spec_from_file_location('b', '../build.py'); m = u.module_from_spec(s); s.loader.exec_module(m); print(' '.join(x[:-4] for x in m.SOURCES))")
for f in $SOURCES; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -DMLH_STAGE_CLOCK -I../../include -c $f.hip -o ../lib/dbg/$f.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/libmloam_hip_dbg.so ../lib/dbg/*.o -ldl
