#!/bin/bash
# Same-box A/B on the ViT-g GEMM shapes and the RAFT stage: the current build vs another build of libvtgb.so (see tools/ab_bench.sh;
# nothing is overwritten).
#   tools/ab_gemm.sh path/to/other.so
cd "${GRAFT_REPO_ROOT:-.}"
OTHER="$1"
if [ -z "$OTHER" ] || [ ! -f "$OTHER" ]; then echo "usage: $0 path/to/other/libvtgb.so" >&2; exit 2; fi
run() {
  echo "== $1"; python tools/gemm_bench.py 992 2>&1 | grep -v amdgpu.ids | tail -6
  python tools/raft_bench.py 31 2>&1 | tail -n 1
}
for i in 1 2; do
  run new
  VTGB_LIB="$(realpath "$OTHER")" run other
done
