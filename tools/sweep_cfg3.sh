# usage: tools/sweep_cfg3.sh OUT_DIR  -- the configs[3] leg (bench.py --full) under each MUGIQ_HIP_CONTRACT_TUNE setting
O=${1:?usage: tools/sweep_cfg3.sh OUT_DIR}
mkdir -p "$O"
# (three fields leave swz at 0: every variant but the default runs without the XCD swizzle; the mixed mode of this leg launches
# workgroups of 256 whatever block is asked for, so the block field only matters to the same-precision legs)
for t in default 256,1,1 256,2,1 256,3,1 128,3,1 512,3,1 512,2,1 256,3,0; do
  if [ $t = default ]; then unset MUGIQ_HIP_CONTRACT_TUNE; else export MUGIQ_HIP_CONTRACT_TUNE=$t; fi
  python bench.py --full --steps 2 --warmup 1 --extra cfg3 --no-cpu-baseline > "$O/b_$t.json" 2> "$O/b_$t.err" || exit 1
  echo "$t done"
done
