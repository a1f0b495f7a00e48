#!/bin/bash
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 500 python bench.py --full > $OUT/r3_final_bench.json 2> $OUT/r3_final_bench.err; cut -c1-400 $OUT/r3_final_bench.json
timeout -k 10 500 python bench.py --full --paired --steps 2 --warmup 1 > $OUT/r3_final_paired.json 2> $OUT/r3_final_paired.err; cut -c1-300 $OUT/r3_final_paired.json
timeout -k 10 500 python bench.py --full --long --steps 1 --warmup 1 > $OUT/r3_final_long.json 2> $OUT/r3_final_long.err; cut -c1-300 $OUT/r3_final_long.json
