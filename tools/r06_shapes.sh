mkdir -p gpurun_out/r06s
export REPS=3000
cat gpurun_out/r06s/power5.txt
