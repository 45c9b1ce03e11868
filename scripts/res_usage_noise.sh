#!/bin/bash
# register / spill / LDS use of every k_noisy, k_noisy_hbm, k_noisy_accept, k_noisy_hbm_accept, k_noisy*_k2* and k_noisy*_dyn* instantiation (cross-compile, no GPU needed): DESIGN.md 5f
#   usage: scripts/res_usage_noise.sh [directory that receives the six units' assembly, to compare two builds]
cd "$(dirname "$0")/../qcmrf_amd/csrc" || exit 1
out=$(mktemp -d)
for f in qsv_noise qsv_noise_hbm qsv_noise_measure qsv_noise_accept qsv_noise_kraus2 qsv_noise_dynamic; do
  hipcc -O3 --offload-arch=gfx950 -std=c++17 -munsafe-fp-atomics -Wno-unused-value -Wno-unused-result --cuda-device-only -S \
    -Rpass-analysis=kernel-resource-usage -o "${1:-$out}/$f.s" $f.hip 2> "$out/$f.txt" &
done; wait
cat "$out"/*.txt | grep -E "Function Name|VGPRs:|SGPRs Spill|ScratchSize|Occupancy|LDS Size" | sed 's/.*remark: *//; s/\[-Rpass.*//' \
  | paste - - - - - - | sed 's/Function Name: //' | sort
rm -rf "$out"
