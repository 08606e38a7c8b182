#!/bin/bash
# usage: tools/kernel_resources.sh <file.hip> [name filter]   -- VGPRs / spills / scratch / waves per SIMD / LDS bytes per kernel (gfx950)
f=$1; pat=${2:-.}
root="$(cd "$(dirname "$0")/.." && pwd)"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -I"$root/include" -I"$root/videotgb_amd/csrc" -c "$f" -o /dev/null \
  -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs:|VGPRs Spill|ScratchSize|Occupancy|LDS Size" | sed 's/.*remark: *//; s/ \[-Rpass.*//' | \
  awk '/Function Name/{if(n)print n, v, s, sc, o, l; n=$3} /^VGPRs:/{v="vgpr="$2} /VGPRs Spill/{s="spill="$3} /ScratchSize/{sc="scratch="$NF} /Occupancy/{o="waves="$NF} /LDS Size/{l="lds="$NF} END{print n, v, s, sc, o, l}' | grep -E "$pat"
