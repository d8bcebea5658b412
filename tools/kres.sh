#!/bin/bash
# compact per-kernel resource usage of one HIP source: tools/kres.sh csrc/file.hip [filter]
# one line per kernel: its demangled name with its template arguments | SGPRs, VGPRs, AGPRs, scratch, occupancy, LDS
obj=$(mktemp --suffix=.o)
trap 'rm -f "$obj"' EXIT
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c "$1" -o "$obj" -Rpass-analysis=kernel-resource-usage 2>&1 | \
  grep -E "remark: +(Function Name|TotalSGPRs:|VGPRs:|AGPRs:|ScratchSize|Occupancy|LDS Size)" | \
  sed -E 's/.*remark: +//; s/ \[-Rpass.*//; s/Function Name: //; s/TotalSGPRs/SGPRs/; s/ScratchSize [^:]*/Scratch/; s/Occupancy [^:]*/Waves/; s/LDS Size [^:]*/LDS/' | \
  paste - - - - - - - | while IFS=$'\t' read -r name rest; do
    # the argument list goes, the template arguments stay: "(anonymous namespace)" is the only other parenthesis
    name=$(echo "$name" | c++filt | sed -E 's/^void //; s/\(anonymous namespace\):://g; s/pds:://g; s/\(.*//')
    echo "$name | $(echo "$rest" | tr '\t' ' ')"
  done | grep -E "${2:-.}"
