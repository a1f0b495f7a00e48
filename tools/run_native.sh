#!/bin/bash
# Diagnostic: the bench reference + reads on disk once, then smaltgpu-map under several settings (stage times on stderr).
# usage: tools/run_native.sh <reads> ; settings come from the NATIVE_ENVS variable ("A=1 B=2;C=3"), extra options from NATIVE_ARGS
# NATIVE_FASTA=<columns>: the same reads once more as FASTA wrapped at that many columns, every setting on both files;
# NATIVE_REPEAT=<n>: every setting n times
# (run-to-run spread on one box: 410-560 k reads/s for the same binary, mostly in the first device allocations)
set -e -o pipefail
N=${1:-2000000}
T=$(mktemp -d /tmp/native.XXXX)
python - "$N" "$T" "${NATIVE_FASTA:-0}" <<'PY'
import sys, os
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
from smalt_amd import gpuindex, indexfile
n, tmp, cols = int(sys.argv[1]), sys.argv[2], int(sys.argv[3])
dev = torch.device("cuda", 0)
nchr, chrlen, k, s, rlen = 24, 125000000, 13, 6, 150
sop = np.arange(nchr + 1, dtype=np.int64) * chrlen
ref = gpuindex.make_reference_gpu(nchr, chrlen, 20261004, dev)
packed = gpuindex.pack_reference(ref)
idx, pos = gpuindex.build_perfect_index(ref, sop, k, s)
reads, _ = gpuindex.make_reads_gpu(ref, sop, n, rlen, 777)
rd = reads.cpu().numpy().reshape(n, rlen)
prefix = os.path.join(tmp, "hs")
tot = int(sop[-1])
indexfile.write_sma(prefix, ["chr%d" % (i + 1) for i in range(nchr)], sop, packed.cpu().numpy())
indexfile.write_smi_perfect(prefix, k, s, idx.cpu().numpy(), pos.cpu().numpy(), (tot + s - 1) // s - 1)
q = b"I" * rlen
with open(os.path.join(tmp, "r.fq"), "wb") as f:
    for i in range(n):
        f.write(b"@r%d\n" % i + rd[i].tobytes() + b"\n+\n" + q + b"\n")
if cols:
    with open(os.path.join(tmp, "r.fa"), "wb") as f:
        for i in range(n):
            sq = rd[i].tobytes()
            f.write(b">r%d\n" % i + b"".join(sq[o:o + cols] + b"\n" for o in range(0, rlen, cols)))
PY
IFS=';' read -ra SETS <<< "${NATIVE_ENVS:-X=1}"
FILES="r.fq"
[ -n "$NATIVE_FASTA" ] && FILES="r.fq r.fa"
for f in $FILES; do
for e in "${SETS[@]}"; do
for i in $(seq ${NATIVE_REPEAT:-1}); do
  echo "== $e $f"
  env $e SMALTGPU_MAP_VERBOSE=1 ./smalt_amd/smaltgpu-map -r -1 -f cigar -n 16 $NATIVE_ARGS -o $T/out.cig $T/hs $T/$f 2>&1 | grep smaltgpu-map
  rm -f $T/out.cig
done
done
done
rm -rf $T
