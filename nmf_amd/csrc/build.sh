#!/usr/bin/env bash
# Builds libnmf_hip.so (gfx950 only) and the host extension _nmf_host.so in-tree.  hipcc cross-compiles without a GPU.
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
out="$here/../lib"
mkdir -p "$out"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -fno-fast-math -Wall -Wno-unused-function"
objs=()
for f in "$here"/*.hip; do
  o="$out/$(basename "${f%.hip}").o"
  stale=0
  for h in "$here"/*.hpp "$here/../../include/nmf_hip.h"; do [ "$h" -nt "$o" ] && stale=1; done
  if [ ! -f "$o" ] || [ "$f" -nt "$o" ] || [ "$stale" = 1 ]; then
    extra=""
    # bookkeeping kernels must reproduce the CPU oracle bit-for-bit: no a*b+c -> fma contraction there
    case "$(basename "$f")" in
      march.hip|select.hip|composite.hip|env.hip|metrics.hip|mesh.hip|tv.hip|relight_eval.hip|camera.hip|edit.hip|atlas.hip|compose.hip|accum.hip|denoise.hip) extra="-ffp-contract=off" ;;
      # the MLP backward keeps 128 accumulator registers alive across its loop: transient MFMA results go to VGPRs directly
      # (the default picks the AGPR form for every MFMA of a 512-register kernel and copies each result out)
      brdf_mlp.hip) extra="-mllvm -amdgpu-mfma-vgpr-form=1" ;;
    esac
    # (a failed compile must not leave the previous object to be linked: remove it first, check that all exist afterwards)
    rm -f "$o"
    "$HIPCC" $FLAGS $extra -c "$f" -o "$o" &
  fi
  objs+=("$o")
done
wait
for o in "${objs[@]}"; do
  if [ ! -f "$o" ]; then echo "build.sh: $o was not produced (compile error above)" >&2; exit 1; fi
done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o "$out/libnmf_hip.so"
echo "built $out/libnmf_hip.so"

# The host extension lib/_nmf_host.so (csrc/host_ext.cpp + step_core.inc: the per-step wrappers of hip.py and the fused pass in
# C++, over the same C ABI).  Plain g++ against the torch headers, no device code.  hip.py requires it: a failure fails the build.
ext="$out/_nmf_host.so"
if [ ! -f "$ext" ] || [ "$here/host_ext.cpp" -nt "$ext" ] || [ "$here/step_core.inc" -nt "$ext" ] || [ "$here/../../include/nmf_hip.h" -nt "$ext" ]; then
  tdir="$(python3 -c 'import torch, os; print(os.path.dirname(torch.__file__))')"
  pyinc="$(python3 -c 'import sysconfig; print(sysconfig.get_paths()["include"])')"
  if ! g++ -O2 -fPIC -shared -std=c++17 "$here/host_ext.cpp" \
       -I"$here/../../include" -I"$tdir/include" -I"$tdir/include/torch/csrc/api/include" -I"$pyinc" \
       -D_GLIBCXX_USE_CXX11_ABI=1 -DTORCH_EXTENSION_NAME=_nmf_host \
       -L"$tdir/lib" -ltorch -ltorch_cpu -lc10 -ltorch_python -L"$out" -lnmf_hip \
       -Wl,-rpath,'$ORIGIN' -Wl,-rpath,"$tdir/lib" -o "$ext.tmp" 2> "$out/host_ext.log"; then
    rm -f "$ext.tmp"
    echo "build.sh: the host extension did not compile ($out/host_ext.log ends):" >&2
    tail -n 40 "$out/host_ext.log" >&2
    exit 1
  fi
  mv "$ext.tmp" "$ext"
  echo "built $ext"
fi
