#!/bin/bash
# scripts/profile_bench.sh TAG "<bench args>" [OUTDIR]: on an MI355X, for `python3 bench.py <args>`,
# into OUTDIR (a directory under the repository root, default build/profiles):
#   TAG_bench.json          the bench line of a --full run
#   TAG_kernel_stats.csv    rocprofv3 --kernel-trace --stats summary
#   TAG_pmc_hbm_per_launch.json   FETCH_SIZE / WRITE_SIZE (separate --pmc passes)
# Copy what is to be judged into profiles/ afterwards.
set -o pipefail
tag="$1"; args="$2"; out="${3:-build/profiles}"
root=$PWD
mkdir -p $out
python3 bench.py --full $args > $out/${tag}_bench.json 2> $out/${tag}_bench.err || { tail -20 $out/${tag}_bench.err; exit 1; }
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof_$tag
(cd $root && rocprofv3 --kernel-trace --stats -d /tmp/prof_$tag -o p --output-format csv -- python3 bench.py $args --no-cpu --no-events --no-parity --no-secondary > /tmp/prof_$tag.log 2>&1) || { tail -20 /tmp/prof_$tag.log; exit 1; }
f=$(find /tmp/prof_$tag -name '*kernel_stats.csv' | head -1)
cp "$f" $root/$out/${tag}_kernel_stats.csv
head -6 $root/$out/${tag}_kernel_stats.csv | cut -c1-60,200-
cd $root && bash scripts/pmc.sh "$args --no-parity --no-secondary" $out/${tag}_pmc_hbm_per_launch.json "FETCH_SIZE" "WRITE_SIZE"
