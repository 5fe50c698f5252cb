#!/usr/bin/env bash
# registers / spills / LDS of the observation kernels as the compiler reports them (device-only compile with what
# `build.sh --compile-args UNIT` prints: the build's flags, the unit's defines and its source):
#   tools/kernel_resources.sh [unit ...]      (units of csrc/build.sh's list, fl_obs_m3 / fl_obs_f6 / fl_obs_s4b ...; default: fl_obs_m2 fl_obs_m0 fl_obs_m1)
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
units=("$@"); [ ${#units[@]} -eq 0 ] && units=(fl_obs_m2 fl_obs_m0 fl_obs_m1)
for u in "${units[@]}"; do
  args=$("$ROOT/flatland_marl_amd/csrc/build.sh" --compile-args "$u")
  /opt/rocm/bin/hipcc --cuda-device-only -Rpass-analysis=kernel-resource-usage $args -c -o /dev/null 2>&1 |
    grep -E "Function Name|VGPRs:|SGPRs:|Spill|ScratchSize|LDS Size|Occupancy" | sed 's/.*remark: [^ ]* *//' | paste - - - - - - - - - | sed 's/  */ /g' &
done
wait
